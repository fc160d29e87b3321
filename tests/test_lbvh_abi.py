"""prt_scene_rebuild and prt_scene_rebuild_info: declared in include/prt.h and bound in _native.py under ABI 4
with their line in the header's history, the kernels live in a unit of their own that the build compiles, both
calls refuse a NULL scene without a device, rebuild() refuses a scene that differs in more than its geometry,
rebuild_ratio is refused without refit on the sequence API and on the command line, and the host bookkeeping of a
rebuild runs clean under AddressSanitizer and UBSan in a stand-alone driver (tools/sanitize/lbvh_check.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pyrenderer_amd", "csrc")


def header():
    return open(os.path.join(ROOT, "include", "prt.h")).read()


def test_declared_and_bound():
    from pyrenderer_amd import _native as N
    src = header()
    for name in ("prt_scene_rebuild", "prt_scene_rebuild_info"):
        assert re.search(r"^int %s\(" % name, src, re.M) and name in N.EXPORTS, name
    assert "#define PRT_ABI_VERSION 4" in src and N.ABI_VERSION == 4
    history = src[src.index("ABI history"):src.index("#define PRT_ABI_VERSION")]
    assert "prt_scene_rebuild" in history and "prt_scene_rebuild_info" in history
    assert N.EXPORTS["prt_scene_rebuild"] == N.EXPORTS["prt_scene_update"]      # the same arguments


def test_the_kernels_have_a_unit_of_their_own():
    from pyrenderer_amd import build as B
    assert "prt_lbvh.hip" in B.SOURCES and "prt_lbvh.h" in B.HEADERS
    unit = open(os.path.join(CSRC, "prt_lbvh.hip")).read()
    kernels = set(re.findall(r"^(lbvh_\w+_kernel)\(", unit, re.M))
    assert {"lbvh_centroid_kernel", "lbvh_morton_kernel", "lbvh_keys_kernel", "lbvh_topology_kernel",
            "lbvh_count_kernel", "lbvh_scatter_kernel", "lbvh_emit_kernel"} <= kernels, kernels
    for f in sorted(os.listdir(CSRC)):
        if f != "prt_lbvh.hip":
            assert not re.search(r"lbvh_\w+_kernel", open(os.path.join(CSRC, f)).read()), f
    # the launch interface takes plain device pointers: no scene, no buffer type of the host units
    iface = open(os.path.join(CSRC, "prt_lbvh.h")).read()
    assert "Scene" not in iface and "DevBuf" not in iface and "prt_host.h" not in iface + unit
    # no kernel of the unit waits: no arrival counter, no spin on memory
    assert not re.search(r"\bwhile\s*\([^)]*(atomic|volatile)", unit) and "__threadfence" not in unit


def test_null_scene_is_an_argument_error_without_a_device():
    from pyrenderer_amd import _native as N
    L = N.lib()
    v = np.zeros(9, np.float32)
    assert L.prt_scene_rebuild(None, N.ptr(v), N.ptr(v), None) == N.PRT_ERR_ARG
    assert b"NULL" in L.prt_last_error()
    info, ms = np.zeros(8, np.int64), np.zeros(8, np.float64)
    assert L.prt_scene_rebuild_info(None, N.ptr(info), N.ptr(ms)) == N.PRT_ERR_ARG


class _NoDevice:
    """DeviceScene's checks without a device: the methods under test stop before any library call."""

    def __init__(self, flat):
        from pyrenderer_amd.device_scene import DeviceScene
        self.ds = DeviceScene.__new__(DeviceScene)
        self.ds.flat, self.ds.h, self.ds._built_cost, self.ds.last_update = flat, None, None, None


def test_rebuild_checks_compatibility_first(cornell):
    from pyrenderer_amd.flatten import FlatScene
    flat = cornell[2]
    ds = _NoDevice(flat).ds
    fewer = FlatScene(flat.tri_v[:-1], flat.tri_n[:-1], flat.tri_mat[:-1], flat.tri_prim[:-1], flat.prim_lo, flat.prim_hi,
                      flat.mat, flat.light_tri, flat.light_off, flat.direct_rgb)
    with pytest.raises(ValueError, match="primitive counts"):
        ds.rebuild(fewer)
    other = FlatScene(flat.tri_v, flat.tri_n, flat.tri_mat[::-1].copy(), flat.tri_prim, flat.prim_lo, flat.prim_hi,
                      flat.mat, flat.light_tri, flat.light_off, flat.direct_rgb)
    with pytest.raises(ValueError, match="tri_mat"):
        ds.rebuild(other)
    for bad in (0, -1.0, "3", float("nan")):
        with pytest.raises(ValueError, match="rebuild_ratio"):
            ds.update(flat, rebuild_ratio=bad)
    assert ds.flat is flat and ds.last_update is None


def test_rebuild_ratio_needs_refit(cornell):
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    scene, cam, _ = cornell
    with pytest.raises(ValueError, match="refit=True"):
        TemporalAccumulator(scene, depth=4, spp=1, resolution=(64, 64), rebuild_ratio=3)
    with pytest.raises(ValueError, match="refit=True"):
        render_sequence(scene, [cam], spp=1, depth=4, resolution=(64, 64), refit=False, rebuild_ratio=3)
    with pytest.raises(ValueError, match="rebuild_ratio"):
        TemporalAccumulator(scene, depth=4, spp=1, resolution=(64, 64), refit=True, rebuild_ratio=0)
    acc = TemporalAccumulator(scene, depth=4, spp=1, resolution=(64, 64), refit=True, rebuild_ratio=3)
    assert acc.rebuild_ratio == 3 and acc.refit


def test_rebuild_ratio_flag_needs_refit(capsys):
    from pyrenderer_amd.main import parse
    for argv in (["--frames", "2", "--spin", "5", "6", "--rebuild-ratio", "3"], ["--rebuild-ratio", "3"]):
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--refit" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse(["--frames", "2", "--spin", "5", "6", "--refit", "--rebuild-ratio", "0"])
    assert parse(["--frames", "2", "--spin", "5", "6", "--refit", "--rebuild-ratio", "3"]).rebuild_ratio == 3.0
    assert parse(["--frames", "2", "--spin", "5", "6", "--refit"]).rebuild_ratio is None


def _sanitizer_runtime():
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        return False
    r = subprocess.run([cxx, "-print-file-name=libasan.so"], capture_output=True, text=True)
    return r.returncode == 0 and os.path.isabs(r.stdout.strip())


# slots, seed, distinct codes (0: random 30-bit codes); (nodes4, need4) of the duplicates is DESIGN.md §14's
@pytest.mark.skipif(not _sanitizer_runtime(), reason="no AddressSanitizer runtime for g++")
@pytest.mark.parametrize("args,pinned", [((0, 1), (1, 4)), ((1, 1), (1, 4)), ((3, 1), (1, 4)), ((300, 3, 1), (49, 13)),
                                         ((3000, 4), None), ((20000, 5, 50), None)])
def test_host_bookkeeping_clean_under_asan_ubsan(args, pinned):
    san = os.path.join(ROOT, "tools", "sanitize")
    exe = os.path.join(ROOT, "build", "sanitize", "lbvh_check")
    subprocess.run(["make", "-s", "-C", san, exe], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["failures"] == 0 and rep["slots"] == args[0] and rep["inner"] == max(args[0] - 1, 0), rep
    assert rep["levels4"] >= rep["levels8"] >= 1 and rep["nodes4"] >= rep["nodes8"] >= 1, rep
    if pinned:
        assert (rep["nodes4"], rep["need4"]) == pinned, rep

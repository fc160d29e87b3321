"""The pooled kernel's unit for the eight-wide tree (prt_trace_pool.hip with -DPRT_POOL_WIDTH=8, build.py
POOL_WIDE): the same listing checks as tests/test_isa_kernarg.py makes on the four-wide unit — every
instantiation copies the kernarg segment pointer before anything writes s0 / s1, the production builds
spill no SGPRs — and the lean production build, the one configs 1, 2 and 5 run, fits the 72 VGPRs of
seven waves per SIMD with nothing spilled and no scratch (CPU only, ~10 s)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.skipif(not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_width8_pool_kernel_listing(tmp_path):
    from pyrenderer_amd import build as B
    from tools import isa_kernarg as K
    assert [w for w, _ in B.POOL_WIDE] == [8]
    listing = str(tmp_path / "pool8.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + [f for f in B.FLAGS if f != "-fPIC"] + B.UNIT_FLAGS[B.POOL_UNIT] + [
        "-DPRT_POOL_WIDTH=8", "--cuda-device-only", "-S", os.path.join(B.CSRC, B.POOL_UNIT), "-o", listing]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    kernels = {n: meta for n, _, meta in K.kernels(listing) if "trace_kernel_pool" in n}
    assert len(kernels) == 8 and all(n.endswith("Li8EEEvNS_11TraceParamsE") for n in kernels)
    assert K.check(listing) == []
    lean = [m for n, m in kernels.items() if "ILb0ELi7ELb1ELi8E" in n]   # <STATS false, 7 waves, PLAIN, 8>
    assert len(lean) == 1
    m = lean[0]
    assert int(m["vgpr_count"]) <= 72 and int(m["vgpr_spill_count"]) == 0 and int(m["sgpr_spill_count"]) == 0
    assert int(m["private_segment_fixed_size"]) == 0

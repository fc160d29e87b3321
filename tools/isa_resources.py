"""Resource table of every device kernel of libprt, cross-compiled for gfx950 (CPU only, no GPU needed).

    python tools/isa_resources.py <outdir> [--src <tree>]      (writes <outdir>/resources.txt and the listings)

Compiles the build's device units (the 8 prt_trace_inst.hip sets, prt_trace_pool.hip, prt_kernels.hip and the
denoiser's prt_denoise.hip) with
build.py's flags and per-unit flags plus `--cuda-device-only -S`, and records per kernel: VGPRs, SGPRs,
spilled VGPRs / SGPRs, scratch bytes, static LDS bytes and the instruction count.  `--src` points at another
checkout (e.g. a worktree of the parent commit) to build the table a change is compared with; two tables
are compared with diff.  profiles/r08/shared_shading/ holds the pair of round 8's shared shading pieces.
"""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size"]


def main():
    from pyrenderer_amd import build as B
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--src", default=ROOT, help="checkout whose pyrenderer_amd/csrc is compiled")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    csrc = os.path.join(a.src, "pyrenderer_amd", "csrc")
    units = [(f"trace_{s}_{t}", B.TRACE_INST, [f"-DPRT_STACK={s}", f"-DPRT_STATS={t}"]) for s, t in B.TRACE_SETS]
    units += [(os.path.splitext(f)[0], f, B.UNIT_FLAGS.get(f, [])) for f in ("prt_trace_pool.hip", "prt_kernels.hip", "prt_denoise.hip")]
    # the pooled kernel's units for the wider trees (a parent tree without them has no POOL_WIDE)
    units += [(f"prt_trace_pool{w}", B.POOL_UNIT, B.UNIT_FLAGS[B.POOL_UNIT] + [f"-DPRT_POOL_WIDTH={w}"])
              for w, _ in getattr(B, "POOL_WIDE", []) if a.src == ROOT]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def compile_unit(u):
        name, src, flags = u
        lst = os.path.join(a.out, name + ".s")
        subprocess.run([hipcc] + B.FLAGS + flags + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", lst],
                       check=True, capture_output=True)
        return name, lst

    with ThreadPoolExecutor(B._jobs()) as ex:
        listings = list(ex.map(compile_unit, units))
    rows = []
    for name, lst in listings:
        text = open(lst).read()
        meta = {}
        for block in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
            d = {k: m.group(1) for k in KEYS + [".name"]
                 if (m := re.search(r"^\s*" + re.escape(k) + r":\s*(\S+)", block, re.M))}
            if ".name" in d:
                meta[d[".name"]] = d
        counts, cur = {}, None
        for ln in text.split("\n"):
            m = re.match(r"^(\w+):", ln)
            if m and m.group(1) in meta:
                cur = m.group(1)
                counts[cur] = 0
            elif cur and (ln.startswith(".Lfunc_end") or ln.startswith("\t.section")):
                cur = None
            elif cur:
                t = ln.split(";")[0].strip()
                counts[cur] += bool(t) and not t.startswith(".") and not t.endswith(":")
        names = subprocess.run(["c++filt"], input="\n".join(meta), capture_output=True, text=True).stdout.split("\n")
        for k, pretty in zip(meta, names):
            pretty = re.sub(r"\(.*\)$", "", re.sub(r"prt(_dn)?::\(anonymous namespace\)::", "", pretty).replace("void ", ""))
            rows.append(f"{name} {pretty} {' '.join(meta[k].get(x, '?') for x in KEYS)} {counts.get(k, 0)}")
    table = "# unit kernel vgpr sgpr vgpr_spill sgpr_spill scratch lds insts\n" + "\n".join(sorted(rows)) + "\n"
    open(os.path.join(a.out, "resources.txt"), "w").write(table)
    sys.stdout.write(table)


if __name__ == "__main__":
    main()

"""Time the a-trous filter (prt_denoise_device) with HIP events: warm-up, then the median of
repeated enqueues on one stream.  Inputs: an 8-spp Cornell render and its
features at 512^2, tiled to the larger sizes.  One JSON line per size.

    python tools/denoise_time.py --sizes 512 4096
    python tools/denoise_time.py --mode variance --sizes 512 4096   # the variance-guided mode (prt_denoise_var_device)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mode", choices=("fixed", "variance"), default="fixed")
    a = ap.parse_args()
    import torch
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import build_world, render
    from pyrenderer_amd.io_utils.read_tungsten import read_file

    scene, cam = read_file(os.path.join(ROOT, "pyrenderer_amd", "media", "cornell-box", "scene.json"))
    world = build_world(scene, (0,))
    base = 512
    noisy = render(scene, cam, spp=8, depth=8, seed=2, resolution=(base, base), world=world)
    feat = D.features(scene, cam, resolution=(base, base), samples=1, seed=2, world=world)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for size in a.sizes:
        k = (size + base - 1) // base
        c = np.ascontiguousarray(np.tile(noisy, (k, k, 1))[:size, :size])
        f = np.ascontiguousarray(np.tile(feat, (k, k, 1))[:size, :size])
        d_c, d_f = torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev)
        d_out = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        variance = a.mode == "variance"
        need = D.work_bytes_variance(size, size) if variance else D.work_bytes(size, size)
        d_work = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def run():
            if variance:
                D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), size, size, d_out.data_ptr(), d_work.data_ptr(),
                                          need, iterations=a.iterations, stream_ptr=stream.cuda_stream)
                return
            D.denoise_device(d_c.data_ptr(), d_f.data_ptr(), size, size, d_out.data_ptr(), d_work.data_ptr(), need,
                             iterations=a.iterations, stream_ptr=stream.cuda_stream)

        for _ in range(a.warmup):
            run()
        stream.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        n = size * size
        # compulsory traffic: per pass one read of the packed planes (two float4 + the float2 gradient) and
        # one write of I (float4); the pre-pass reads colour + features and writes the planes, the post-pass
        # reads I, the class plane, colour and albedo and writes the colour
        per_pass = n * (16 + 16 + 8 + 16)
        fixed = n * ((12 + 32 + 16 + 16 + 8) + (16 + 16 + 12 + 32 + 12))
        what = "denoise_time"
        if variance:
            # per pass one read of (I, var), (N, class), the gradient and the depth and one write of (I, var); the
            # estimate reads (I, Z), (N, class) and the gradient and writes (I, var) and the depth
            per_pass = n * (16 + 16 + 8 + 4 + 16)
            fixed += n * ((16 + 16 + 8) + (16 + 4))
            what = "denoise_var_time"
        total = per_pass * a.iterations + fixed
        print(json.dumps(dict(what=what, size=size, iterations=a.iterations, median_ms=round(med, 4),
                              min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=a.reps,
                              bytes_per_pass=per_pass, bytes_total=total,
                              implied_gbs=round(total / (med * 1e-3) / 1e9, 1),
                              hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))), flush=True)
        del d_c, d_f, d_out, d_work


if __name__ == "__main__":
    main()

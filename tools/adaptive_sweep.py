"""What adaptive sampling buys: AdaptiveAccumulator against a uniform render of no fewer samples.

For the Cornell box and scene_specular.json at 128^2 and 512^2, batches of 8 spp, at most --max-batches of
them and three targets: the adaptive render's share of the sample budget, and its error against a
--ref-spp render of the same frame beside that of render(spp=n) with n the adaptive render's mean samples per
pixel rounded UP (so the uniform render never has fewer samples in total).  Two errors per image: the RMSE of
the whole frame, and the worst 64 x 64 tile's RMSE, which is what a noise target is about.  The yardstick is
the --ref-spp render, never the sampler's own estimate.  The ratios are printed as measured.

    python tools/adaptive_sweep.py > profiles/adaptive_sweep.txt
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.denoise_sweep import load, rmse   # noqa: E402

TILE = 64


def tile_rmse(img, ref):
    """RMSE per 64 x 64 tile of the frame, (tiles_x, tiles_y)."""
    W, H = img.shape[:2]
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out = np.zeros((tx, ty))
    for i in range(tx):
        for j in range(ty):
            r = (slice(i * TILE, (i + 1) * TILE), slice(j * TILE, (j + 1) * TILE))
            out[i, j] = rmse(img[r], ref[r])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--targets", type=float, nargs="+", default=[0.2, 0.1, 0.05])
    ap.add_argument("--batch-spp", type=int, default=8)
    ap.add_argument("--max-batches", type=int, default=32)
    ap.add_argument("--tolerate", type=float, default=0.0)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--ref-spp", type=int, default=4096)
    a = ap.parse_args()
    from pyrenderer_amd.adaptive import AdaptiveAccumulator
    from pyrenderer_amd.core.tracing import build_world, render

    print(f"# adaptive sampling against uniform sampling: batches of {a.batch_spp} spp, at most {a.max_batches} "
          f"({a.batch_spp * a.max_batches} spp), tolerate {a.tolerate:g}, depth {a.depth}, seed {a.seed}; errors against "
          f"{a.ref_spp} spp (seed {a.seed + 1000})")
    print("# share = samples spent / budget; uniform = render(spp) with spp = ceil(adaptive mean spp);")
    print("# ratio = adaptive RMSE / uniform RMSE (below 1: adaptive is better at no more samples)")
    print(f"{'scene':9s}{'size':>5s}{'target':>8s}{'share':>8s}{'tiles':>12s}{'mean spp':>10s}{'uni spp':>8s}"
          f"{'frame ad':>10s}{'frame un':>10s}{'ratio':>7s}{'worst ad':>10s}{'worst un':>10s}{'ratio':>7s}{'s ad':>7s}{'s un':>7s}")
    for which in ("cornell", "specular"):
        scene, cam = load(which)
        world = build_world(scene, (0,))
        for size in a.sizes:
            kw = dict(depth=a.depth, resolution=(size, size), world=world)
            ref = render(scene, cam, spp=a.ref_spp, seed=a.seed + 1000, **kw).astype(np.float64)
            for target in a.targets:
                t0 = time.perf_counter()
                acc = AdaptiveAccumulator(scene, cam, batch_spp=a.batch_spp, target=target, tolerate=a.tolerate,
                                          seed=a.seed, **kw).run(a.max_batches)
                img = acc.mean()
                t_ad = time.perf_counter() - t0
                mean_spp = float(acc.samples().mean())
                spp_u = int(math.ceil(mean_spp))
                t0 = time.perf_counter()
                uni = render(scene, cam, spp=spp_u, seed=a.seed, **kw)
                t_un = time.perf_counter() - t0
                per = acc.batches_per_tile
                f_ad, f_un = rmse(img, ref), rmse(uni, ref)
                w_ad, w_un = tile_rmse(img, ref).max(), tile_rmse(uni, ref).max()
                print(f"{which:9s}{size:5d}{target:8.3f}{acc.spent(a.max_batches):8.3f}"
                      f"{f'{int(per.min())}..{int(per.max())}':>12s}{mean_spp:10.2f}{spp_u:8d}{f_ad:10.5f}{f_un:10.5f}"
                      f"{f_ad / f_un:7.3f}{w_ad:10.5f}{w_un:10.5f}{w_ad / w_un:7.3f}{t_ad:7.2f}{t_un:7.2f}", flush=True)


if __name__ == "__main__":
    main()

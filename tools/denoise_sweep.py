"""Parameter sweep of the a-trous denoiser: sigma_c, sigma_z, eps_a, eps_z.

For the Cornell box and scene_specular.json at 128^2 and 512^2 with 4, 8 and 64 spp, the score of
a parameter set is the RMSE of the denoised frame against a 4096-spp render of the same frame
(other seed), divided by the noisy frame's RMSE; sets are ranked by the geometric mean of that
ratio over the twelve frames.  The yardstick is the 4096-spp render, never the filter's output.

    python tools/denoise_sweep.py --out profiles/denoise_sweep.txt

--mode variance sweeps the variance-guided mode instead (sigma_l, eps_l, sigma_z; eps_a and eps_z stay
at the fixed filter's defaults) on the same frames with the same score:

    python tools/denoise_sweep.py --mode variance --out profiles/denoise_var_sweep.txt

--mode variance --variance-batches K [K ...] sweeps the same three parameters with the variance taken from
per-pixel moments of K batch means (render_batches) instead of the 7 x 7 estimate, one section per K, on
the spp columns that K divides.  The noisy frame is then the batch-order mean, so each section also scores
the fixed filter's and the spatial estimate's defaults on those very frames:

    python tools/denoise_sweep.py --mode variance --variance-batches 4 8 --spp 4 8 16 32 64 \
        --out profiles/denoise_mom_sweep.txt

--mode temporal sweeps the temporal accumulation's alpha (= alpha_m), tau_z and tau_n on turntables: per
scene, size and spp an orbit of --frames frames at --orbit degrees per frame about the look-at point.  The
score of a set is the RMSE of the last frame (temporal accumulation, then the variance-guided filter with
the spatial fallback) against a --ref-spp render of the last camera, divided by the RMSE of the
variance-guided filter on the last frame alone at the same per-frame spp:

    python tools/denoise_sweep.py --mode temporal --spp 1 4 --ref-spp 1024 --out profiles/denoise_temporal_sweep.txt
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEDIA = os.path.join(ROOT, "pyrenderer_amd", "media", "cornell-box")
SIGMA_C = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
SIGMA_Z = (0.5, 1.0, 2.0, 4.0)
EPS_A = (1e-3, 1e-2, 5e-2)
EPS_Z = (1e-4, 1e-3, 1e-2)
VAR_SIGMA_L = (1.0, 2.0, 4.0, 8.0)
VAR_EPS_L = (1e-4, 1e-3, 1e-2)
VAR_SIGMA_Z = (0.5, 1.0, 2.0)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def load(which):
    from pyrenderer_amd.io_utils.read_tungsten import process_primitives, read_file
    if which == "cornell":
        return read_file(os.path.join(MEDIA, "scene.json"))
    return process_primitives(json.load(open(os.path.join(MEDIA, "scene_specular.json"))))


def sweep_variance(a, frames):
    """The --mode variance leg: table and choice for sigma_l, eps_l, sigma_z."""
    from pyrenderer_amd.denoise import EPS_A, EPS_Z, denoise_variance
    rows = []
    for sl, el, sz in itertools.product(VAR_SIGMA_L, VAR_EPS_L, VAR_SIGMA_Z):
        ratios = [rmse(denoise_variance(n, f, iterations=a.iterations, sigma_l=sl, sigma_z=sz, eps_l=el), r) / e
                  for _, n, f, r, e in frames]
        rows.append((float(np.exp(np.mean(np.log(ratios)))), sl, el, sz, ratios))
    rows.sort(key=lambda t: t[0])
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    print(f"# variance-guided a-trous parameter sweep: iterations {a.iterations}, depth {a.depth}, reference {a.ref_spp} spp "
          f"(seed 1), noisy frames seed 2, eps_a {EPS_A:g}, eps_z {EPS_Z:g}", file=out)
    print("# noisy RMSE: " + "  ".join(f"{n} {e:.5f}" for n, _, _, _, e in frames), file=out)
    print("# columns: geometric-mean ratio, sigma_l, eps_l, sigma_z, then RMSE(denoised) / RMSE(noisy) of "
          + " ".join(f[0] for f in frames), file=out)
    for g, sl, el, sz, ratios in rows:
        print(f"{g:.4f} {sl:g} {el:g} {sz:g}  " + " ".join(f"{r:.4f}" for r in ratios), file=out)
    if out is not sys.stdout:
        out.close()
    g, sl, el, sz, _ = rows[0]
    print(f"best: sigma_l {sl:g} eps_l {el:g} sigma_z {sz:g} (geometric-mean ratio {g:.4f})")
    safe = [r for r in rows if max(r[4]) < 1.0]
    if safe:
        g, sl, el, sz, ratios = safe[0]
        print(f"best with every frame improved: sigma_l {sl:g} eps_l {el:g} sigma_z {sz:g} "
              f"(geometric-mean ratio {g:.4f}, worst frame {max(ratios):.4f})")
    else:
        g, sl, el, sz, ratios = min(rows, key=lambda t: max(t[4]))
        print(f"no set improves every frame; best worst frame: sigma_l {sl:g} eps_l {el:g} sigma_z {sz:g} "
              f"(geometric-mean ratio {g:.4f}, worst frame {max(ratios):.4f})")


TEMPORAL_ALPHA = (0.1, 0.2, 0.4)
TEMPORAL_TAU_Z = (0.01, 0.02, 0.05)
TEMPORAL_TAU_N = (0.8, 0.9, 0.95)


def sweep_temporal(a):
    """The --mode temporal leg: table and choice for alpha, tau_z, tau_n."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.camera import orbit
    from pyrenderer_amd.core.tracing import _Frame, _mean, build_world, render
    seqs = []   # (name, [(mean, feat, cam record)] per frame, reference, RMSE of the spatial-only filter)
    for which in ("cornell", "specular"):
        scene, cam = load(which)
        world = build_world(scene, (0,))
        cams = [orbit(cam, a.orbit * t) for t in range(a.frames)]
        for size in a.sizes:
            res = (size, size)
            ref = render(scene, cams[-1], spp=a.ref_spp, depth=a.depth, seed=1, resolution=res, world=world)
            for spp in a.spp:
                frames = []
                for t, c in enumerate(cams):   # frame t: samples t * spp ..., as TemporalAccumulator.add renders it
                    f = _Frame.of(scene, c, depth=a.depth, seed=2, resolution=res, world=world)
                    frames.append((_mean(f.unpack(f.add_samples(t * spp, spp)), spp), f.features(), f.cam))
                alone = D.denoise_variance(frames[-1][0], frames[-1][1], iterations=a.iterations)
                seqs.append((f"{which}-{size}-{spp}spp", frames, ref, rmse(alone, ref), rmse(frames[-1][0], ref)))
            print(f"rendered {which} {size}", file=sys.stderr, flush=True)

    def last_frame(frames, **par):
        prev = None
        for mean, feat, rec in frames:
            state, color = D.temporal_accumulate(mean, feat, rec, prev, **par)
            prev = (state, feat, rec)
        return D.denoise_variance(color, feat, iterations=a.iterations, variance=state[..., 6],
                                  variance_fallback="spatial"), state

    rows = []
    for al, tz, tn in itertools.product(TEMPORAL_ALPHA, TEMPORAL_TAU_Z, TEMPORAL_TAU_N):
        ratios, shares = [], []
        for _, frames, ref, e_alone, _ in seqs:
            img, state = last_frame(frames, alpha=al, alpha_m=al, tau_z=tz, tau_n=tn)
            hit = frames[-1][1][..., 7] > 0
            ratios.append(rmse(img, ref) / e_alone)
            shares.append(float((state[..., 3][hit] > 1).mean()))
        rows.append((float(np.exp(np.mean(np.log(ratios)))), al, tz, tn, ratios, min(shares)))
    rows.sort(key=lambda t: t[0])
    names = [q[0] for q in seqs]
    n_c = sum(n.startswith("cornell") for n in names)   # the Cornell sequences come first
    gm = lambda v: float(np.exp(np.mean(np.log(v))))
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    print(f"# temporal accumulation parameter sweep: {a.frames} frames at {a.orbit:g} degrees per frame, iterations "
          f"{a.iterations}, depth {a.depth}, reference {a.ref_spp} spp of the last camera (seed 1), frames seed 2, "
          f"alpha_m = alpha, tau_a {D.TEMPORAL_TAU_A:g}, min_history {D.TEMPORAL_MIN_HISTORY:g}, w_min {D.TEMPORAL_W_MIN:g}, "
          f"filter defaults", file=out)
    print("# last frame, unfiltered RMSE: " + "  ".join(f"{q[0]} {q[4]:.5f}" for q in seqs), file=out)
    print("# last frame, variance-guided filter alone RMSE: " + "  ".join(f"{q[0]} {q[3]:.5f}" for q in seqs), file=out)
    print("# columns: geometric-mean ratio, the same over the Cornell sequences, alpha, tau_z, tau_n, least share of hit "
          "pixels with history in a last frame, then RMSE(temporal + filter) / RMSE(filter alone) of " + " ".join(names),
          file=out)
    for g, al, tz, tn, ratios, share in rows:
        print(f"{g:.4f} {gm(ratios[:n_c]):.4f} {al:g} {tz:g} {tn:g} {share:.4f}  " + " ".join(f"{r:.4f}" for r in ratios),
              file=out)
    if out is not sys.stdout:
        out.close()
    g, al, tz, tn, ratios, _ = rows[0]
    print(f"best: alpha {al:g} tau_z {tz:g} tau_n {tn:g} (geometric-mean ratio {g:.4f}, worst sequence {max(ratios):.4f})")
    safe = [r for r in rows if max(r[4]) < 1.0]
    if safe:
        g, al, tz, tn, ratios, _ = safe[0]
        print(f"best with no sequence worse than the filter alone: alpha {al:g} tau_z {tz:g} tau_n {tn:g} "
              f"(geometric-mean ratio {g:.4f}, worst sequence {max(ratios):.4f})")
    else:
        on_c = sorted((r for r in rows if max(r[4][:n_c]) < 1.0), key=lambda r: gm(r[4][:n_c]))
        print("no set keeps every sequence below the filter alone" + (
            f"; on the Cornell sequences alone: alpha {on_c[0][1]:g} tau_z {on_c[0][2]:g} tau_n {on_c[0][3]:g} "
            f"(geometric-mean ratio {gm(on_c[0][4][:n_c]):.4f}, worst {max(on_c[0][4][:n_c]):.4f})" if on_c else ""))


def sweep_moments(a):
    """The --variance-batches leg: per K a table for sigma_l, eps_l, sigma_z with the moments' variance."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import build_world, render, render_batches
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    worlds = {}
    for which in ("cornell", "specular"):
        scene, cam = load(which)
        world = build_world(scene, (0,))
        worlds[which] = (scene, cam, world, {size: render(scene, cam, spp=a.ref_spp, depth=a.depth, seed=1,
                                                          resolution=(size, size), world=world) for size in a.sizes})
        print(f"rendered {which} references", file=sys.stderr, flush=True)
    for K in a.variance_batches:
        frames = []
        for which, (scene, cam, world, refs) in worlds.items():
            for size in a.sizes:
                for spp in (s for s in a.spp if s >= K and s % K == 0):
                    sums, feat, state = render_batches(scene, cam, spp=spp, depth=a.depth, variance_batches=K, seed=2,
                                                       resolution=(size, size), world=world)
                    noisy = sums / np.float32(spp)
                    frames.append((f"{which}-{size}-{spp}spp", noisy, feat, refs[size], rmse(noisy, refs[size]),
                                   np.ascontiguousarray(state[..., 3])))
        rows = []
        for sl, el, sz in itertools.product(VAR_SIGMA_L, VAR_EPS_L, VAR_SIGMA_Z):
            ratios = [rmse(D.denoise_variance(n, f, iterations=a.iterations, sigma_l=sl, sigma_z=sz, eps_l=el, variance=v), r) / e
                      for _, n, f, r, e, v in frames]
            rows.append((float(np.exp(np.mean(np.log(ratios)))), sl, el, sz, ratios))
        rows.sort(key=lambda t: t[0])
        fixed = [rmse(D.denoise(n, f, iterations=a.iterations), r) / e for _, n, f, r, e, _ in frames]
        spatial = [rmse(D.denoise_variance(n, f, iterations=a.iterations), r) / e for _, n, f, r, e, _ in frames]
        default = next(r for r in rows if (r[1], r[2], r[3]) == (D.VAR_SIGMA_L, D.VAR_EPS_L, D.VAR_SIGMA_Z))
        gm = lambda v: float(np.exp(np.mean(np.log(v))))
        print(f"# K = {K}: variance of the mean from {K} batch means; iterations {a.iterations}, depth {a.depth}, "
              f"reference {a.ref_spp} spp (seed 1), noisy frames seed 2 (batch-order mean), eps_a {D.EPS_A:g}, "
              f"eps_z {D.EPS_Z:g}", file=out)
        print("# frames: " + " ".join(f[0] for f in frames), file=out)
        print("# noisy RMSE: " + "  ".join(f"{f[0]} {f[4]:.5f}" for f in frames), file=out)
        print(f"# fixed default    {gm(fixed):.4f} worst {max(fixed):.4f}  " + " ".join(f"{r:.4f}" for r in fixed), file=out)
        print(f"# spatial default  {gm(spatial):.4f} worst {max(spatial):.4f}  " + " ".join(f"{r:.4f}" for r in spatial), file=out)
        print(f"# moments default  {default[0]:.4f} worst {max(default[4]):.4f}  " + " ".join(f"{r:.4f}" for r in default[4]), file=out)
        print("# columns: geometric-mean ratio, sigma_l, eps_l, sigma_z, then RMSE(denoised) / RMSE(noisy) per frame", file=out)
        for g, sl, el, sz, ratios in rows:
            print(f"{g:.4f} {sl:g} {el:g} {sz:g}  " + " ".join(f"{r:.4f}" for r in ratios), file=out)
        out.flush()
        safe = [r for r in rows if max(r[4]) < 1.0]
        print(f"K {K}: fixed {gm(fixed):.4f} spatial {gm(spatial):.4f} moments default {default[0]:.4f} best {rows[0][:4]}"
              + (f" best with every frame improved {safe[0][:4]} worst {max(safe[0][4]):.4f}" if safe else " (no set improves every frame)"))
    if out is not sys.stdout:
        out.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="-", help="table file ('-' = stdout)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--spp", type=int, nargs="+", default=[4, 8, 64])
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--mode", choices=("fixed", "variance", "temporal"), default="fixed",
                    help="fixed: sigma_c, sigma_z, eps_a, eps_z of denoise(); variance: sigma_l, eps_l, sigma_z of "
                         "denoise_variance(); temporal: alpha, tau_z, tau_n of temporal_accumulate() on turntables")
    ap.add_argument("--frames", type=int, default=8, help="--mode temporal: frames per turntable")
    ap.add_argument("--orbit", type=float, default=2.0, help="--mode temporal: degrees per frame")
    ap.add_argument("--variance-batches", type=int, nargs="+", default=[], metavar="K",
                    help="with --mode variance: take the variance from K batch means (one section per K)")
    a = ap.parse_args()
    if a.variance_batches:
        if a.mode != "variance" or min(a.variance_batches) < 2:
            ap.error("--variance-batches needs --mode variance and K >= 2")
        return sweep_moments(a)
    if a.mode == "temporal":
        return sweep_temporal(a)
    from pyrenderer_amd.core.tracing import build_world, render
    from pyrenderer_amd.denoise import denoise, features

    frames = []
    for which in ("cornell", "specular"):
        scene, cam = load(which)
        world = build_world(scene, (0,))
        for size in a.sizes:
            res = (size, size)
            ref = render(scene, cam, spp=a.ref_spp, depth=a.depth, seed=1, resolution=res, world=world)
            feat = features(scene, cam, resolution=res, samples=1, seed=2, world=world)
            for spp in a.spp:
                noisy = render(scene, cam, spp=spp, depth=a.depth, seed=2, resolution=res, world=world)
                frames.append((f"{which}-{size}-{spp}spp", noisy, feat, ref, rmse(noisy, ref)))
            print(f"rendered {which} {size}", file=sys.stderr, flush=True)

    if a.mode == "variance":
        return sweep_variance(a, frames)

    rows = []
    for sc, sz, ea, ez in itertools.product(SIGMA_C, SIGMA_Z, EPS_A, EPS_Z):
        ratios = [rmse(denoise(n, f, iterations=a.iterations, sigma_c=sc, sigma_z=sz, eps_a=ea, eps_z=ez), r) / e
                  for _, n, f, r, e in frames]
        rows.append((float(np.exp(np.mean(np.log(ratios)))), sc, sz, ea, ez, ratios))
    rows.sort(key=lambda t: t[0])

    out = sys.stdout if a.out == "-" else open(a.out, "w")
    names = [f[0] for f in frames]
    print(f"# a-trous parameter sweep: iterations {a.iterations}, depth {a.depth}, reference {a.ref_spp} spp (seed 1), "
          f"noisy frames seed 2", file=out)
    print("# noisy RMSE: " + "  ".join(f"{n} {e:.5f}" for n, _, _, _, e in frames), file=out)
    print("# columns: geometric-mean ratio, sigma_c, sigma_z, eps_a, eps_z, then RMSE(denoised) / RMSE(noisy) of "
          + " ".join(names), file=out)
    for g, sc, sz, ea, ez, ratios in rows:
        print(f"{g:.4f} {sc:g} {sz:g} {ea:g} {ez:g}  " + " ".join(f"{r:.4f}" for r in ratios), file=out)
    if out is not sys.stdout:
        out.close()
    g, sc, sz, ea, ez, _ = rows[0]
    print(f"best: sigma_c {sc:g} sigma_z {sz:g} eps_a {ea:g} eps_z {ez:g} (geometric-mean ratio {g:.4f})")
    # a default must not make any frame of the sweep worse than its input
    safe = [r for r in rows if max(r[5]) < 1.0]
    if safe:
        g, sc, sz, ea, ez, ratios = safe[0]
        print(f"best with every frame improved: sigma_c {sc:g} sigma_z {sz:g} eps_a {ea:g} eps_z {ez:g} "
              f"(geometric-mean ratio {g:.4f}, worst frame {max(ratios):.4f})")


if __name__ == "__main__":
    main()

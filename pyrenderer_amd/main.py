"""Command-line renderer: the build's counterpart of the reference's render scripts
(main_taichi.py:15-127 — read_file, World, PathTracer, progressive render() passes with a
samples/s print, finish() tone map, out.png every 100 passes; main.py:107-125's
--samples flag), without the Taichi GUI.

    python -m pyrenderer_amd [scene.json] --samples 64 --depth 16 --out out.png
    python -m pyrenderer_amd --samples 256 --interval 32 --state acc.npz      # resumable
    python -m pyrenderer_amd --samples 64 --devices 0 1 2 3                   # tiles over 4 GPUs
    python -m pyrenderer_amd --samples 8 --denoise --aov aov/                 # filtered image + feature buffers
    python -m pyrenderer_amd --samples 8 --denoise --denoise-mode variance    # width from the image's own noise
    python -m pyrenderer_amd --samples 64 --denoise --denoise-mode variance --variance-batches 8   # ... from sample moments
    python -m pyrenderer_amd --samples 2 --frames 24 --orbit 2 --temporal --denoise --denoise-mode variance   # turntable
    python -m pyrenderer_amd --samples 2 --frames 24 --spin 5 6 --temporal --denoise --denoise-mode variance    # a box turns
    python -m pyrenderer_amd --adaptive 0.05 --batch-spp 8 --max-samples 256              # until the noise is below 5 %

Every sample runs through libprt's HIP path (core.tracing.render / Accumulator); there is
no CPU fallback.
"""
import argparse
import functools
import os
import time

import numpy as np

from . import denoise as D
from .core.camera import orbit
from .core.tracing import Accumulator, TemporalAccumulator, _check_variance_batches, _Frame, _mean, as_image
from .io_utils.read_tungsten import read_file
from .tone_map import finish, reinhard_extended, save_hdr, to_uint8, write_png

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SCENE = os.path.join(HERE, "media", "cornell-box", "scene.json")


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pyrenderer_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("scene", nargs="?", default=DEFAULT_SCENE, help="Tungsten scene.json (default: Cornell box)")
    ap.add_argument("--samples", type=int, default=64, help="samples per pixel (main_taichi.py:29)")
    ap.add_argument("--depth", type=int, default=16, help="path depth (main_taichi.py:37)")
    ap.add_argument("--resolution", type=int, nargs=2, metavar=("W", "H"), help="override camera.resolution")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--devices", type=int, nargs="+", default=[0], help="GPUs of this process (tiles shard over them)")
    ap.add_argument("--nee", choices=["reference", "mis"], default="reference",
                    help="direct lighting: sample_direct_lighting (reference) or sample_direct_lighting2 (MIS)")
    ap.add_argument("--interval", type=int, default=0,
                    help="progressive passes of this many spp with a samples/s line each (one device; 0 = one pass)")
    ap.add_argument("--state", help="progressive accumulation file: resumed when it exists, saved after every pass")
    ap.add_argument("--tonemap", choices=["sqrt", "reinhard"], default="sqrt",
                    help="finish() = sqrt(pixels/samples) (main_taichi.py:61-64) or finishing_tonemap (:67-78)")
    ap.add_argument("--out", default="out.png", help="PNG path ('' = no image)")
    ap.add_argument("--hdr", metavar="DIR",
                    help="also save the reference's HDR pair (main_taichi.py:120-123) into DIR: hdr.npy = the "
                         "radiance sums (W, H, 3) [x][y], spp.npy = the per-pixel sample counts (W, H); "
                         "the reference's tone_map.py reads exactly these")
    ap.add_argument("--denoise", action="store_true",
                    help="filter the image with the edge-avoiding a-trous denoiser (pyrenderer_amd.denoise), guided "
                         "by one-sample first-hit albedo / normal / depth; --hdr still saves the raw sums")
    ap.add_argument("--denoise-iterations", type=int, default=None, metavar="N",
                    help="a-trous passes, 0..8 (default 5; pass i uses step 2^i); implies --denoise")
    ap.add_argument("--denoise-mode", choices=("fixed", "variance"), default="fixed",
                    help="with --denoise: 'fixed' (default) stops at colour edges with one fixed width; 'variance' "
                         "takes the width from a per-pixel estimate of the image's own noise")
    ap.add_argument("--variance-batches", type=int, default=0, metavar="K",
                    help="with --denoise --denoise-mode variance: take the variance from per-pixel moments of K "
                         "batch means instead of the spatial estimate (0 = off, else >= 2; --samples must be a "
                         "multiple of K).  With --interval every pass is a batch (K only switches the moments on) "
                         "and --samples must be a multiple of the interval; the moments are used from 4 batches on")
    ap.add_argument("--aov", metavar="DIR",
                    help="save the first-hit feature buffers into DIR: albedo.png, normal.png (0.5 n + 0.5) and "
                         "depth.npy ((W, H) float32 [x][y], 0 where no ray hits); with --denoise --denoise-mode "
                         "variance also variance.npy, the (W, H) float32 variance of the demodulated luminance "
                         "that the filter used (the spatial estimate, or with --variance-batches the sample moments')")
    ap.add_argument("--frames", type=int, default=0, metavar="N",
                    help="render N frames of --samples spp each and write out.0000.png ...; with --orbit the camera "
                         "turns between them (0 = one image, the default)")
    ap.add_argument("--orbit", type=float, default=0.0, metavar="DEG",
                    help="with --frames: turn the scene's camera about its look-at point around its up vector by "
                         "DEG degrees per frame")
    ap.add_argument("--temporal", action="store_true",
                    help="with --frames: carry the previous frame's colour and luminance moments into the next "
                         "camera (temporal accumulation); filtered with --denoise --denoise-mode variance, or "
                         "written as accumulated without --denoise")
    ap.add_argument("--spin", nargs=2, default=None, metavar=("PRIM", "DEG"),
                    help="with --frames: turn primitive PRIM (its index in the scene) by DEG degrees per frame about "
                         "the vertical axis through the centre of its bounding box; with --temporal the history "
                         "follows it (per-object motion and an object-id test); usable with --orbit 0")
    ap.add_argument("--refit", action="store_true",
                    help="with --frames and --spin: refit the resident scene's BVH on the GPU between frames instead "
                         "of building a new scene per frame (same images)")
    ap.add_argument("--rebuild-ratio", type=float, default=None, metavar="R",
                    help="with --refit: build the resident scene's BVH again on the GPU once refits have raised "
                         "its tree cost above R times the value at the last build (same images); no default, "
                         "DESIGN.md section 14 has the measured break-even")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TARGET",
                    help="adaptive sampling: render in batches of --batch-spp and stop every 64 x 64 tile once the "
                         "relative standard error of its pixels' demodulated luminance is at most TARGET; needs "
                         "--batch-spp and --max-samples (--samples is not used); one device, one image")
    ap.add_argument("--batch-spp", type=int, default=None, metavar="N", help="with --adaptive: samples per batch")
    ap.add_argument("--max-samples", type=int, default=None, metavar="M",
                    help="with --adaptive: the most samples a pixel gets, a multiple of --batch-spp")
    ap.add_argument("--min-batches", type=int, default=None, metavar="B",
                    help="with --adaptive: batches every tile gets before it may stop (default 2, the least)")
    ap.add_argument("--tolerate", type=float, default=None, metavar="F",
                    help="with --adaptive: the share of a tile's pixels, in [0, 1), that may stay over TARGET "
                         "(default 0)")
    args = ap.parse_args(argv)
    _check_adaptive(ap, args)
    if args.denoise_iterations is not None:
        if not 0 <= args.denoise_iterations <= 8:
            ap.error(f"--denoise-iterations must be in 0..8, not {args.denoise_iterations}")
        args.denoise = True
    try:   # render()'s rules; with --interval every pass is a batch, whatever K is
        _check_variance_batches(args.variance_batches, None if args.interval > 0 else args.samples,
                                "variance" if args.denoise and args.denoise_mode == "variance" else args.denoise,
                                args.devices)
    except ValueError as e:
        ap.error(f"--variance-batches: {e}")
    if args.variance_batches:
        if args.interval > 0:
            if args.samples % args.interval:
                ap.error(f"--variance-batches with --interval {args.interval} needs --samples to be a multiple of it "
                         f"(equal batches), not {args.samples}")
        elif args.state:
            ap.error("--variance-batches with --state needs --interval (every pass is a batch)")
    if args.frames < 0:
        ap.error(f"--frames must be >= 0, not {args.frames}")
    if args.spin is not None:
        try:
            args.spin = (int(args.spin[0]), float(args.spin[1]))
        except ValueError:
            ap.error(f"--spin takes a primitive index and degrees per frame, not {args.spin[0]!r} {args.spin[1]!r}")
        if args.spin[0] < 0 or not np.isfinite(args.spin[1]):
            ap.error(f"--spin needs a primitive index >= 0 and finite degrees, not {args.spin[0]} {args.spin[1]}")
    if args.refit and args.spin is None:
        ap.error("--refit refits the scene that --spin moves: it needs --frames N --spin PRIM DEG")
    if args.rebuild_ratio is not None and not args.refit:
        ap.error("--rebuild-ratio rebuilds the scene that --refit keeps resident: it needs --refit")
    if args.rebuild_ratio is not None and not (np.isfinite(args.rebuild_ratio) and args.rebuild_ratio > 0):
        ap.error(f"--rebuild-ratio needs a finite ratio > 0, not {args.rebuild_ratio}")
    if not args.frames:
        for flag, given in (("--orbit", args.orbit != 0.0), ("--temporal", args.temporal), ("--spin", args.spin),
                            ("--refit", args.refit)):
            if given:
                ap.error(f"{flag} needs --frames N")
    else:
        clash = [flag for flag, given in (("--interval", args.interval > 0), ("--state", args.state),
                                          ("--variance-batches", args.variance_batches), ("--hdr", args.hdr),
                                          ("--aov", args.aov), ("--devices", len(args.devices) != 1)) if given]
        if clash:
            ap.error(f"--frames renders whole frames on one device: it cannot be combined with {', '.join(clash)}")
        if args.samples < 1:
            ap.error(f"--frames needs --samples >= 1 per frame, not {args.samples}")
        if args.temporal and args.denoise and args.denoise_mode != "variance":
            ap.error("--temporal feeds the variance-guided filter: use --denoise --denoise-mode variance, or no "
                     "--denoise at all")
    if args.hdr and args.hdr.lower().endswith(".npy"):
        # rounds <= 4 took a .npy FILE here; a directory named out.npy would silently replace it
        ap.error(f"--hdr takes a directory (hdr.npy and spp.npy are written into it), not a .npy file: {args.hdr}")
    return args


def _check_adaptive(ap, args):
    """--adaptive and its companions: complete, in range, and combined with nothing that renders otherwise."""
    companions = (("--batch-spp", args.batch_spp), ("--max-samples", args.max_samples),
                  ("--min-batches", args.min_batches), ("--tolerate", args.tolerate))
    if args.adaptive is None:
        for flag, value in companions:
            if value is not None:
                ap.error(f"{flag} needs --adaptive TARGET")
        return
    clash = [flag for flag, given in (("--devices", len(args.devices) != 1), ("--interval", args.interval > 0),
                                      ("--variance-batches", args.variance_batches), ("--temporal", args.temporal),
                                      ("--frames", args.frames), ("--state", args.state), ("--spin", args.spin)) if given]
    if clash:
        ap.error(f"--adaptive renders one image in batches on one device and keeps its own moments: it cannot be "
                 f"combined with {', '.join(clash)}")
    if args.batch_spp is None or args.max_samples is None:
        ap.error("--adaptive needs --batch-spp N and --max-samples M")
    args.min_batches = 2 if args.min_batches is None else args.min_batches
    args.tolerate = 0.0 if args.tolerate is None else args.tolerate
    try:
        from .adaptive import check_sampler   # the sampler's own rules; imports torch
        check_sampler(args.batch_spp, args.adaptive, args.min_batches, args.tolerate, 1.0)
    except ValueError as e:
        ap.error(f"--adaptive: {e}")
    if args.max_samples < args.batch_spp or args.max_samples % args.batch_spp:
        ap.error(f"--adaptive: --max-samples ({args.max_samples}) must be a positive multiple of --batch-spp "
                 f"({args.batch_spp})")


def render_adaptively(args, scene, camera, W, H):
    """--adaptive: an AdaptiveAccumulator run to --max-samples, with the share of the samples it spent printed."""
    from .adaptive import AdaptiveAccumulator
    acc = AdaptiveAccumulator(scene, camera, depth=args.depth, batch_spp=args.batch_spp, target=args.adaptive,
                              min_batches=args.min_batches, tolerate=args.tolerate, seed=args.seed,
                              resolution=(W, H), device=args.devices[0], nee=args.nee)
    max_batches = args.max_samples // args.batch_spp
    acc.run(max_batches)
    per_tile = acc.batches_per_tile
    print(f"adaptive: target {args.adaptive:g}, {acc.batches} of {max_batches} batches of {args.batch_spp} spp; "
          f"{100.0 * acc.spent(max_batches):.1f} % of {args.max_samples} spp per pixel spent "
          f"(tiles: {int(per_tile.min())}..{int(per_tile.max())} batches, {int(acc.active.sum())} of "
          f"{per_tile.shape[0]} still over the target)", flush=True)
    return acc


def write_aov(directory, feat):
    """--aov: albedo.png, normal.png (0.5 n + 0.5) and depth.npy of a features() array."""
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, n) for n in ("albedo.png", "normal.png", "depth.npy")]
    write_png(paths[0], to_uint8(as_image(feat[..., 0:3])))
    write_png(paths[1], to_uint8(as_image(np.float32(0.5) * feat[..., 3:6] + np.float32(0.5))))
    np.save(paths[2], np.ascontiguousarray(feat[..., 6]))
    return paths


def _write(args, sums, samples, mean):
    if args.hdr:
        save_hdr(args.hdr, sums, samples)
    if args.out:
        img = finish(mean) if args.tonemap == "sqrt" else reinhard_extended(mean)
        write_png(args.out, to_uint8(as_image(img)))


def frame_path(out, t):
    """--frames: out.png -> out.0000.png for frame t."""
    root, ext = os.path.splitext(out)
    return f"{root}.{t:04d}{ext}"


def render_frames(args, scene, camera, W, H):
    """--frames N --orbit DEG [--spin PRIM DEG] [--temporal]: one image per camera; returns the last frame's mean."""
    from .core.tracing import build_world
    scenes = None
    if args.spin is not None:
        from .scenes import spun
        try:
            scenes = spun(scene, args.spin[0], args.spin[1], args.frames)
        except ValueError as e:
            raise SystemExit(f"--spin: {e}")
    # --refit: one world of the sequence's own, updated in place (the accumulator builds its own)
    refit = args.refit and scenes is not None   # parse() refuses --refit without --spin
    world = None if refit and args.temporal else build_world(scene, (args.devices[0],))
    it = D.ITERATIONS if args.denoise_iterations is None else args.denoise_iterations
    acc = None
    if args.temporal:
        acc = TemporalAccumulator(scene, depth=args.depth, spp=args.samples, seed=args.seed, resolution=(W, H),
                                  device=args.devices[0], world=world, nee=args.nee, refit=refit,
                                  rebuild_ratio=args.rebuild_ratio if refit else None)
    mean = None
    for t in range(args.frames):
        cam = orbit(camera, t * args.orbit)
        t0 = time.perf_counter()
        if acc is not None:
            acc.add(cam, None if scenes is None else scenes[t])
            mean = acc.denoised(iterations=it) if args.denoise else acc.accumulated()
        else:
            if refit and t > 0:
                world.update(scenes[t].primitives, rebuild_ratio=args.rebuild_ratio)
            elif scenes is not None and t > 0:   # every frame stands alone, in its own world
                for ds in world.device_scenes.values():
                    ds.close()
                world = build_world(scenes[t], (args.devices[0],))
            frame = _Frame.of(scene, cam, depth=args.depth, seed=args.seed, resolution=(W, H),
                              devices=(args.devices[0],), world=world, nee=args.nee)
            mean = _mean(frame.unpack(frame.add_samples(t * args.samples, args.samples)), args.samples)
            if args.denoise:
                mean = frame.filter(mean, args.denoise_mode, iterations=it)
        if args.out:
            img = finish(mean) if args.tonemap == "sqrt" else reinhard_extended(mean)
            write_png(frame_path(args.out, t), to_uint8(as_image(img)))
        dt = time.perf_counter() - t0
        print(f"frame {t}: {t * args.orbit:g} deg, {dt:.2f} s, mean RGB {mean.mean(axis=(0, 1))}", flush=True)
    return mean


def main(argv=None):
    args = parse(argv)
    scene, camera = read_file(args.scene)
    W, H = args.resolution if args.resolution else camera.resolution
    if args.frames:
        return render_frames(args, scene, camera, W, H)
    t0 = time.perf_counter()
    adaptive_samples = None
    if args.adaptive is not None:
        acc = render_adaptively(args, scene, camera, W, H)
        adaptive_samples = acc.samples()
        sums, samples, mean, denoised = acc.sums(), adaptive_samples, acc.mean(), acc.denoised
    elif args.interval > 0 or args.state:
        if len(args.devices) != 1:
            raise SystemExit("progressive rendering (--interval/--state) runs on one device")
        state = Accumulator.state_path(args.state) if args.state else None
        if state and os.path.exists(state):
            acc = Accumulator.load(state, scene, camera, device=args.devices[0])
            # the saved estimator settings win; refuse a command line that asks for others
            given = {"depth": args.depth, "seed": args.seed, "resolution": (W, H),
                     "nee": args.nee}
            saved = {"depth": acc.frame.depth, "seed": acc.frame.seed, "resolution": (acc.frame.W, acc.frame.H),
                     "nee": "mis" if acc.frame.flags else "reference"}
            clash = [f"--{k} {given[k]} (saved: {saved[k]})" for k in given if given[k] != saved[k]]
            if clash:
                raise SystemExit(f"{state} was rendered with other settings: " + ", ".join(clash))
            if bool(args.variance_batches) != acc.moments:
                raise SystemExit(f"{state} was saved {'with' if acc.moments else 'without'} sample moments: "
                                 f"{'add' if acc.moments else 'drop'} --variance-batches")
            if acc.moments and acc.batch_spp and acc.batch_spp != args.interval:
                raise SystemExit(f"{state} holds batches of {acc.batch_spp} spp: --interval must be {acc.batch_spp}")
            print(f"resumed {state}: {acc.samples} spp")
        else:
            acc = Accumulator(scene, camera, depth=args.depth, seed=args.seed, resolution=(W, H),
                              device=args.devices[0], nee=args.nee, moments=bool(args.variance_batches))
        frame, W, H = acc.frame, acc.frame.W, acc.frame.H
        step = args.interval if args.interval > 0 else args.samples
        while acc.samples < args.samples:
            n = min(step, args.samples - acc.samples)
            t = time.perf_counter()
            acc.add(n)
            dt = time.perf_counter() - t
            print(f"{n / dt:.2f} samples/s ({acc.samples} spp, {W * H * n / dt / 1e6:.1f} Msamples/s)", flush=True)
            if state:
                acc.save(state)
        sums, samples, mean, denoised = acc.sums(), acc.samples, acc.mean(), acc.denoised
    else:
        frame = _Frame.of(scene, camera, depth=args.depth, seed=args.seed, resolution=(W, H),
                          devices=tuple(args.devices), nee=args.nee)
        samples, variance = max(args.samples, 0), None
        if args.variance_batches:
            sums, _, mstate = frame.batches(samples, args.variance_batches)
            variance = mstate[..., 3]
        else:
            sums = frame.sums(samples)
        mean = _mean(sums, samples)
        denoised = functools.partial(frame.filter, mean, variance=variance)
    if args.aov:
        write_aov(args.aov, acc.features() if adaptive_samples is not None else frame.features())
        if adaptive_samples is not None:
            np.save(os.path.join(args.aov, "samples.npy"), adaptive_samples)
    if args.denoise:
        it = D.ITERATIONS if args.denoise_iterations is None else args.denoise_iterations
        mean, var = denoised(args.denoise_mode, iterations=it, return_variance=True)
        if args.aov and var is not None:
            np.save(os.path.join(args.aov, "variance.npy"), var)
    dt = time.perf_counter() - t0
    _write(args, sums, samples, mean)
    spent = args.samples if adaptive_samples is None else round(float(adaptive_samples.mean()), 2)
    print(f"{W}x{H} x {spent} spp, depth {args.depth}: {dt:.2f} s "
          f"({W * H * spent / dt / 1e6:.1f} Msamples/s incl. scene build), mean RGB {mean.mean(axis=(0, 1))}")
    return mean


if __name__ == "__main__":
    main()

"""Time the a-trous filter (prt_denoise_device) with HIP events: warm-up, then the median of
repeated enqueues on one stream.  Inputs: an 8-spp Cornell render and its
features at 512^2, tiled to the larger sizes.  One JSON line per size.

    python tools/denoise_time.py --sizes 512 4096
    python tools/denoise_time.py --mode variance --sizes 512 4096   # the variance-guided mode (prt_denoise_var_device)
    python tools/denoise_time.py --mode given --sizes 512 4096      # ... with a given variance plane (prt_denoise_var_given_device)
    python tools/denoise_time.py --mode moments --sizes 512 4096    # prt_moments_add_device over --frames frames (default 8)
    python tools/denoise_time.py --mode adaptive --sizes 512 4096   # prt_adaptive_update_device, tile 64: every tile, and every other one
    python tools/denoise_time.py --mode batching                    # render(spp=64) against 8 batches of 8, host wall clock, 512^2
    python tools/denoise_time.py --mode features --sizes 512 4096   # prt_features_device (1 and 8 samples); host wall clock of both compositions at 512^2
    python tools/denoise_time.py --temporal --sizes 512 4096        # prt_temporal_accumulate_device, its motion form, and beside them the filter with and without the spatial fallback
    python tools/denoise_time.py --temporal --ab-lib abtmp/libprt_parent.so   # ... and both entry points of another build of the library, alternating
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak
HBM_COPY_GBS = 6290.0   # ... and what a float4 copy reaches of it


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mode", choices=("fixed", "variance", "given", "moments", "adaptive", "batching", "features"),
                    default="fixed")
    ap.add_argument("--frames", type=int, default=8, help="--mode moments: n_frames per call")
    ap.add_argument("--temporal", action="store_true",
                    help="time the temporal accumulation (a camera turned by 2 degrees) and the variance-guided filter "
                         "that follows it")
    ap.add_argument("--ab-lib", metavar="PATH",
                    help="--temporal: another build of libprt.so whose prt_temporal_accumulate_device and its motion form "
                         "are timed in alternation with this build's, --ab-rounds times each")
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import build_world, render
    from pyrenderer_amd.io_utils.read_tungsten import read_file

    scene, cam = read_file(os.path.join(ROOT, "pyrenderer_amd", "media", "cornell-box", "scene.json"))
    world = build_world(scene, (0,))
    base = 512
    if a.mode == "batching":
        return time_batching(a, scene, cam, world)
    if a.mode == "features":
        return time_features(a, cam, world)
    if a.temporal:
        return time_temporal(a, scene, cam, world)
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
        if a.mode == "moments":
            time_moments(a, size, c, d_f, stream)
            continue
        if a.mode == "adaptive":
            time_adaptive(a, size, c, d_f, stream)
            continue
        variance = a.mode in ("variance", "given")
        d_iv = torch.from_numpy(D.denoise_variance(c, f, iterations=0, return_variance=True)[1]).to(dev) if a.mode == "given" else None
        need = D.work_bytes_variance(size, size) if variance else D.work_bytes(size, size)
        d_work = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def run():
            if variance:
                D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), size, size, d_out.data_ptr(), d_work.data_ptr(),
                                          need, iterations=a.iterations, stream_ptr=stream.cuda_stream,
                                          d_in_var_ptr=d_iv.data_ptr() if d_iv is not None else None)
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
        if a.mode == "given":
            # var_given_kernel reads (I, Z), the class plane and the variance and writes (I, var) and the depth
            fixed += n * ((16 + 16 + 4) + (16 + 4)) - n * ((16 + 16 + 8) + (16 + 4))
            what = "denoise_var_given_time"
        total = per_pass * a.iterations + fixed
        print(json.dumps(dict(what=what, size=size, iterations=a.iterations, median_ms=round(med, 4),
                              min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=a.reps,
                              bytes_per_pass=per_pass, bytes_total=total,
                              implied_gbs=round(total / (med * 1e-3) / 1e9, 1),
                              hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))), flush=True)
        del d_c, d_f, d_out, d_work


def _median_ms(run, stream, warmup, reps):
    import torch
    for _ in range(warmup):
        run()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms


def time_moments(a, size, c, d_f, stream):
    """prt_moments_add_device over a.frames packed frames of sums (the 8-spp mean times 8, perturbed per frame)."""
    import torch
    from pyrenderer_amd import denoise as D
    dev = d_f.device
    k = a.frames
    scale = torch.linspace(0.5, 1.5, k, device=dev).reshape(k, 1, 1, 1)
    d_s = (torch.from_numpy(c).to(dev)[None] * 8.0 * scale).contiguous()
    d_state = torch.zeros((size, size, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def run():
        D.moments_add_device(d_s.data_ptr(), k, 8.0, d_f.data_ptr(), size, size, d_state.data_ptr(),
                             stream_ptr=stream.cuda_stream)

    ms = _median_ms(run, stream, a.warmup, a.reps)
    med = ms[len(ms) // 2]
    n = size * size
    total = n * (k * 12 + 32 + 16 + 16)   # the frames and the features read, the state read and written
    print(json.dumps(dict(what="moments_add_time", size=size, n_frames=k, median_ms=round(med, 4), min_ms=round(ms[0], 4),
                          max_ms=round(ms[-1], 4), reps=a.reps, bytes_total=total,
                          implied_gbs=round(total / (med * 1e-3) / 1e9, 1),
                          hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))), flush=True)


def time_adaptive(a, size, c, d_f, stream, tile=64):
    """prt_adaptive_update_device on one batch (the 8-spp mean times 8): the full tile list, and every other
    tile of the frame (a checkerboard of the tile grid, in ascending order).  The yardstick is the traffic the
    kernel must move per listed pixel, 12 B of batch, 28 B of sums and state read and 28 B written and 16 of the
    32 B of features (84 B), over the HBM rates of MI355X_MICROARCH.md: the 8 TB/s peak and the 6.29 TB/s a
    float4 copy measures."""
    import torch
    from pyrenderer_amd.adaptive import adaptive_update_device
    dev = d_f.device
    tx, ty = (size + tile - 1) // tile, (size + tile - 1) // tile
    every = np.arange(tx * ty, dtype=np.int32)
    lists = (("full", every), ("half", every[((every % tx) + (every // tx)) % 2 == 0]))
    d_frame = torch.from_numpy(c).to(dev) * 8.0
    d_sum = torch.zeros((size, size, 3), dtype=torch.float32, device=dev)
    d_state = torch.zeros((size, size, 4), dtype=torch.float32, device=dev)
    for name, ids in lists:
        # the batch in slot order: tile-major, then row ly, then column lx (frames are [x][y])
        pad = torch.zeros((tx * tile, ty * tile, 3), dtype=torch.float32, device=dev)
        pad[:size, :size] = d_frame
        slots = pad.reshape(tx, tile, ty, tile, 3).permute(2, 0, 3, 1, 4).reshape(tx * ty, tile * tile * 3)
        d_b = slots[torch.from_numpy(ids.astype(np.int64)).to(dev)].contiguous()
        d_rec = torch.zeros((len(ids), 4), dtype=torch.int32, device=dev)
        del pad, slots
        torch.cuda.synchronize(dev)

        def run():
            adaptive_update_device(d_b.data_ptr(), ids, tile, tile, size, size, d_f.data_ptr(), 8.0, d_sum.data_ptr(),
                                   d_state.data_ptr(), d_rec.data_ptr(), target=0.05, stream_ptr=stream.cuda_stream)

        ms = _median_ms(run, stream, a.warmup, a.reps)
        med = ms[len(ms) // 2]
        rec = d_rec.cpu().numpy()
        n = int(rec[:, 0].sum())   # the listed pixels inside the frame
        total = n * (12 + 28 + 28 + 16)
        print(json.dumps(dict(what="adaptive_update_time", size=size, tile=tile, tiles=name, n_tiles=len(ids),
                              listed_pixels=n, median_ms=round(med, 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4),
                              reps=a.reps, bytes_total=total, implied_gbs=round(total / (med * 1e-3) / 1e9, 1),
                              hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                              hbm_copy_fraction=round(total / (med * 1e-3) / 1e9 / HBM_COPY_GBS, 4))), flush=True)
        del d_b, d_rec


def time_temporal(a, scene, cam, world):
    """prt_temporal_accumulate_device per size: features of the scene's camera and of the camera turned by 2
    degrees, both rendered at the size itself (the gather follows a real reprojection), an 8-spp colour tiled
    from 512^2, and the previous state of a first frame.  In the same run the variance-guided filter on the
    result: with its own estimate, and with the temporal plane and the spatial fallback."""
    import torch
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.camera import orbit
    from pyrenderer_amd.core.tracing import render
    base = 512
    noisy = render(scene, cam, spp=8, depth=8, seed=2, resolution=(base, base), world=world)
    ds = world.device_scene(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    turned = orbit(cam, 2.0)
    for size in a.sizes:
        k = (size + base - 1) // base
        n = size * size
        d_c = torch.from_numpy(np.ascontiguousarray(np.tile(noisy, (k, k, 1))[:size, :size])).to(dev)
        recs = [c.convert_to_taichi_camera().packed() for c in (cam, turned)]
        d_feats = [torch.empty((size, size, D.FEATURE_CHANNELS), dtype=torch.float32, device=dev) for _ in recs]
        for rec, d_f in zip(recs, d_feats):
            D.features_device(ds, rec, size, size, d_f.data_ptr(), samples=1, seed=2)
        d_states = [torch.empty((size, size, D.TEMPORAL_CHANNELS), dtype=torch.float32, device=dev) for _ in recs]
        d_col = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        d_var = torch.empty((size, size), dtype=torch.float32, device=dev)
        d_out = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        need = D.work_bytes_variance(size, size)
        d_work = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        # a first frame with min_history 1 leaves a state whose every hit pixel donates
        D.temporal_accumulate_device(d_c.data_ptr(), d_feats[0].data_ptr(), recs[0], size, size, d_states[0].data_ptr())
        torch.cuda.synchronize(dev)

        def temporal():
            D.temporal_accumulate_device(d_c.data_ptr(), d_feats[1].data_ptr(), recs[1], size, size, d_states[1].data_ptr(),
                                         d_prev_feat_ptr=d_feats[0].data_ptr(), prev_cam=recs[0],
                                         d_prev_state_ptr=d_states[0].data_ptr(), d_out_color_ptr=d_col.data_ptr(),
                                         d_out_var_ptr=d_var.data_ptr(), min_history=1.0, stream_ptr=stream.cuda_stream)

        def filt(**kw):
            D.denoise_variance_device(d_col.data_ptr(), d_feats[1].data_ptr(), size, size, d_out.data_ptr(),
                                      d_work.data_ptr(), need, iterations=a.iterations, stream_ptr=stream.cuda_stream, **kw)

        # the motion leg: the middle third of the frame (a band in x) carries a non-identity row, a turn of one
        # degree about the vertical axis through the box's centre and a shift of 1 cm; both id planes are the band
        band = ((np.arange(size) * 3) // size == 1).astype(np.int32)
        d_ids = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(band[:, None], (size, size)))).to(dev)
        t = np.radians(1.0)
        rows = np.tile(D.IDENTITY_ROW, (3, 1))
        rot = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
        centre = np.array([0.0, 1.0, 0.0])
        rows[1] = np.concatenate([rot, (centre - rot @ centre + (0.01, 0.0, 0.0))[:, None]], 1).reshape(12)
        d_rows = torch.from_numpy(rows.astype(np.float32)).to(dev)
        torch.cuda.synchronize(dev)

        def temporal_motion():
            D.temporal_accumulate_device(d_c.data_ptr(), d_feats[1].data_ptr(), recs[1], size, size, d_states[1].data_ptr(),
                                         d_prev_feat_ptr=d_feats[0].data_ptr(), prev_cam=recs[0],
                                         d_prev_state_ptr=d_states[0].data_ptr(), d_out_color_ptr=d_col.data_ptr(),
                                         d_out_var_ptr=d_var.data_ptr(), min_history=1.0, stream_ptr=stream.cuda_stream,
                                         d_ids_ptr=d_ids.data_ptr(), d_prev_ids_ptr=d_ids.data_ptr(),
                                         d_motion_ptr=d_rows.data_ptr(), n_objects=3)

        if a.ab_lib:
            time_temporal_ab(a, size, (temporal, temporal_motion), stream, d_c, d_feats, recs, d_states, d_col, d_var, d_ids,
                             d_rows)
        legs = (("temporal_motion_time", temporal_motion, n * 164),
                ("temporal_time", temporal, n * 156),
                ("denoise_var_time", filt, None),
                ("denoise_var_mixed_time", lambda: filt(d_in_var_ptr=d_var.data_ptr(), variance_fallback="spatial"), None))
        valid = None
        for what, run, total in legs:
            ms = _median_ms(run, stream, a.warmup, a.reps)
            med = ms[len(ms) // 2]
            row = dict(what=what, size=size, median_ms=round(med, 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4),
                       reps=a.reps)
            if what in ("temporal_time", "temporal_motion_time"):
                # the motion form reads 4 B of id and, shared between neighbours like the other tap planes, 4 B of
                # previous id on top; the 36 B table stays in cache
                # compulsory traffic: colour 12, features 32, the previous state 32 and features 32 read (each tap
                # plane once: neighbouring pixels share their taps), state 32, colour 12 and variance 4 written
                st = d_states[1].cpu().numpy()
                hit = d_feats[1].cpu().numpy()[..., 7] > 0
                valid = float((st[..., 3][hit] > 1).mean())
                row.update(bytes_total=total, implied_gbs=round(total / (med * 1e-3) / 1e9, 1),
                           hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           hit_pixels_with_history=round(valid, 4))
                if what == "temporal_motion_time":
                    row.update(pixels_with_a_row=round(float(band.mean()), 4))
            else:
                row.update(iterations=a.iterations)
            print(json.dumps(row), flush=True)
        del d_c, d_feats, d_states, d_col, d_var, d_out, d_work, d_ids, d_rows


def time_temporal_ab(a, size, front_ends, stream, d_c, d_feats, recs, d_states, d_col, d_var, d_ids, d_rows):
    """prt_temporal_accumulate_device and prt_temporal_accumulate_motion_device of this build and of the build at
    a.ab_lib on the same buffers, a.ab_rounds times each in alternation: whether a change to the unit left the
    kernels' times alone.  Three legs a round: this build through the Python front end (front_ends: the two calls
    of time_temporal), this build straight through ctypes, the other build straight through ctypes (its front end
    is not at hand).  The HIP events bracket the host's enqueue too, so the first leg against the third carries
    the front end's Python as well (about 2 us); the second against the third compares the libraries alone."""
    import ctypes
    from pyrenderer_amd import _native as N
    from pyrenderer_amd import denoise as D
    other, other_name = ctypes.CDLL(os.path.abspath(a.ab_lib)), os.path.basename(a.ab_lib)
    par = np.array([D.TEMPORAL_ALPHA, D.TEMPORAL_ALPHA_M, D.TEMPORAL_TAU_N, D.TEMPORAL_TAU_Z, D.TEMPORAL_TAU_A, D.EPS_A,
                    1.0, D.TEMPORAL_W_MIN], np.float32)
    vp = ctypes.c_void_p
    for moving, front_end in zip((False, True), front_ends):
        name = "prt_temporal_accumulate" + ("_motion" if moving else "") + "_device"
        motion = (vp(d_ids.data_ptr()), vp(d_ids.data_ptr()), vp(d_rows.data_ptr()), d_rows.shape[0]) if moving else ()

        def bare(lib):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = N.EXPORTS[name]

            def run():
                rc = fn(0, vp(d_c.data_ptr()), vp(d_feats[1].data_ptr()), N.ptr(recs[1]), vp(d_feats[0].data_ptr()),
                        N.ptr(recs[0]), vp(d_states[0].data_ptr()), *motion, size, size, N.ptr(par),
                        vp(d_states[1].data_ptr()), vp(d_col.data_ptr()), vp(d_var.data_ptr()), vp(stream.cuda_stream))
                assert rc == 0, rc
            return run

        legs = (("this", "libprt.so", "front end", front_end), ("this", "libprt.so", "ctypes", bare(N.lib())),
                ("other", other_name, "ctypes", bare(other)))
        for r in range(a.ab_rounds):
            for build, lib_name, how, run in legs:
                ms = _median_ms(run, stream, a.warmup, a.reps)
                print(json.dumps(dict(what="temporal_motion_time_ab" if moving else "temporal_time_ab", build=build,
                                      lib=lib_name, call=how, round=r, size=size,
                                      median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4),
                                      max_ms=round(ms[-1], 4), reps=a.reps)), flush=True)


def time_features(a, cam, world):
    """prt_features_device (features_kernel) on Cornell with HIP events, per size and for 1 and 8 samples: the
    kernel's only compulsory traffic is its 32-B store per pixel, so the implied store bandwidth against
    the HBM peak tells whether the stores or the traversal set the time.  Then the host wall clock at 512^2,
    one sample, of features_packed (the kernel, synchronous, with its device-to-host copy) and
    features_packed_host (the composition it replaced), taken in alternation."""
    import time
    import torch
    from pyrenderer_amd import denoise as D
    ds, cam_packed = world.device_scene(0), cam.convert_to_taichi_camera().packed()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    for size in a.sizes:
        d_f = torch.empty((size, size, D.FEATURE_CHANNELS), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        for samples in (1, 8):
            def run():
                D.features_device(ds, cam_packed, size, size, d_f.data_ptr(), samples=samples, seed=2,
                                  stream_ptr=stream.cuda_stream)

            ms = _median_ms(run, stream, a.warmup, a.reps)
            ds.check_faults()
            med = ms[len(ms) // 2]
            n = size * size
            total = n * 4 * D.FEATURE_CHANNELS
            print(json.dumps(dict(what="features_time", size=size, samples=samples, median_ms=round(med, 4),
                                  min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=a.reps, bytes_stored=total,
                                  implied_store_gbs=round(total / (med * 1e-3) / 1e9, 1),
                                  hbm_peak_fraction=round(total / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                  mrays_per_s=round(n * samples / (med * 1e-3) / 1e6, 1))), flush=True)
        del d_f
    legs = {"features_packed": lambda: D.features_packed(ds, cam_packed, 512, 512, samples=1, seed=2, tile=64),
            "features_packed_host": lambda: D.features_packed_host(ds, cam_packed, 512, 512, samples=1, seed=2, tile=64)}
    t = {k: [] for k in legs}
    warm, reps = 2, 9
    for i in range(warm + reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= warm:
                t[k].append((time.perf_counter() - t0) * 1e3)
    out = dict(what="features_host_wall_time", size=512, samples=1, reps=reps)
    for k, v in t.items():
        out[k + "_ms"] = dict(median=round(sorted(v)[len(v) // 2], 3), min=round(min(v), 3), max=round(max(v), 3))
    print(json.dumps(out), flush=True)


def time_batching(a, scene, cam, world):
    """Host wall clock at 512^2, 64 spp, of the calls around variance_batches=8, taken in alternation (all
    are synchronous): render() without a filter and render(denoise="variance"), the two unbatched paths
    that the moments leave as they were; render(denoise="variance", variance_batches=8); and the
    one-sample feature composition that both filtered calls contain."""
    import time
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import render
    kw = dict(spp=64, depth=8, seed=2, resolution=(512, 512), world=world)
    ds, cam_packed = world.device_scene(0), cam.convert_to_taichi_camera().packed()
    legs = {"render": lambda: render(scene, cam, **kw),
            "render_variance": lambda: render(scene, cam, denoise="variance", **kw),
            "render_variance_batches8": lambda: render(scene, cam, denoise="variance", variance_batches=8, **kw),
            "features": lambda: D.features_packed(ds, cam_packed, 512, 512, samples=1, seed=2, tile=64)}
    t = {k: [] for k in legs}
    warm, reps = 2, 9
    for i in range(warm + reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= warm:
                t[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    out = dict(what="render_batching_time", size=512, spp=64, batches=8, reps=reps)
    for k in legs:
        out[k + "_ms"] = dict(median=round(med[k], 2), min=round(min(t[k]), 2), max=round(max(t[k]), 2))
    out["batched_minus_unbatched_ms"] = round(med["render_variance_batches8"] - med["render_variance"], 2)
    out["batched_over_unbatched"] = round(med["render_variance_batches8"] / med["render_variance"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

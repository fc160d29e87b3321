"""Measurements of the device rebuild against the only rebuild there was before it, a new
DeviceScene: JSON lines on stdout, kept in profiles/refit/.  Medians, one process.

    python tools/rebuild_time.py [--out profiles/refit/rebuild_time.jsonl] [--skip-cubes]

  rebuild    per scene (Cornell, Cornell + a 20 000-triangle soup, instanced_cubes()): wall time of
             DeviceScene.rebuild() and its split (host checks and packing, uploads, codes, sort, binary tree, wide
             emission with its per-level read-backs, triangle records and boxes, quantiser:
             prt_scene_rebuild_info, the kernel groups by HIP events), against DeviceScene(flat) + close() in the
             same process; `faster` says whether rebuild() won; the trees' sizes and stack needs
  quality    the device-built tree against the host-built one on the same pose, and for §13's degradation poses
             the refit, the device-built and the host-built tree: BVH node visits per query (the STATS words) and
             trace-kernel ms per frame (256 x 256, 4 spp, depth 4, the global-scene kernel for the soups and the
             cubes, the default kernel for Cornell), tree_cost() against creation's
  breakeven  from the quality lines of a pose: frames after which a rebuild has paid for itself,
             rebuild ms / (refit frame ms - rebuilt frame ms)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyrenderer_amd import _native as N  # noqa: E402
from pyrenderer_amd import scenes as S  # noqa: E402
from pyrenderer_amd.device_scene import DeviceScene, interleaved_tiles  # noqa: E402
from pyrenderer_amd.flatten import flatten_scene  # noqa: E402
from pyrenderer_amd.io_utils.read_tungsten import read_file  # noqa: E402
from pyrenderer_amd.main import DEFAULT_SCENE  # noqa: E402
from tools.refit_time import displaced, soup, visits_per_query  # noqa: E402

STAGES = ("host_pack", "upload", "codes", "sort", "binary_tree", "wide_emit", "boxes", "quantise")


def time_rebuild(name, flat, moved, reps):
    create = []
    for _ in range(reps):
        t0 = time.perf_counter()
        DeviceScene(moved, 0).close()
        create.append(time.perf_counter() - t0)
    ds = DeviceScene(flat, 0)
    ds.rebuild(moved)                    # the first rebuild allocates its work arrays: not timed
    wall, split = [], []
    for k in range(reps):
        target = flat if k % 2 == 0 else moved
        t0 = time.perf_counter()
        N.check(N.lib().prt_scene_rebuild(ds.h, N.ptr(target.tri_v), N.ptr(target.tri_n),
                                          N.ptr(target.sph if target.sph.shape[0] else None)))
        wall.append(time.perf_counter() - t0)
        split.append(ds.rebuild_info()["ms"])
    info = ds.rebuild_info()
    ds.close()
    s = np.median(np.array(split), axis=0)
    c, u = 1e3 * float(np.median(create)), 1e3 * float(np.median(wall))
    return dict(kind="rebuild", scene=name, triangles=int(flat.n_tri), reps=reps, create_close_ms=round(c, 3),
                rebuild_ms=round(u, 3), ratio=round(c / u, 2), faster=bool(u < c),
                split_ms={k: round(float(v), 3) for k, v in zip(STAGES, s)},
                tree={k: info[k] for k in ("nodes4", "depth4", "need4", "nodes8", "depth8", "need8", "lds_width")})


def frame_ms(ds, cam, W, spp, depth, variant, reps=5):
    ids = interleaved_tiles(W, W, 64)
    flags = N.PRT_FLAG_TIME | (variant << 8)
    ds.render_tiles(cam, W, W, 64, 64, ids, spp, depth, 1, flags)       # warm-up
    ds.kernel_timing()
    out = []
    for _ in range(reps):
        ds.render_tiles(cam, W, W, 64, 64, ids, spp, depth, 1, flags)
        ms, n = ds.kernel_timing()
        out.append(ms)
    return float(np.median(out))


def quality(ds, cam, cost0, variant):
    return dict(visits_per_query=round(visits_per_query(ds, cam, 256, 4, 4), 3),
                frame_ms=round(frame_ms(ds, cam, 256, 4, 4, variant), 4), tree_cost_ratio=round(ds.tree_cost() / cost0, 4),
                stack=ds.kernel_info()["stack"])


def quality_line(label, base, pose, cam, variant, rebuild_ms):
    """The three trees of `pose`: `base`'s tree refit to it (None when pose is base), built on the device, built
    on the host."""
    ds = DeviceScene(base, 0)
    cost0 = ds.tree_cost()
    line = dict(kind="quality", case=label, triangles=int(base.n_tri), variant=variant)
    if pose is not base:
        ds.update(pose)
        line["refit"] = quality(ds, cam, cost0, variant)
    ds.rebuild(pose)
    line["device_built"] = quality(ds, cam, cost0, variant)
    ds.close()
    fresh = DeviceScene(pose, 0)
    line["host_built"] = quality(fresh, cam, cost0, variant)
    fresh.close()
    line["device_over_host_visits"] = round(line["device_built"]["visits_per_query"] / line["host_built"]["visits_per_query"], 4)
    line["device_over_host_ms"] = round(line["device_built"]["frame_ms"] / line["host_built"]["frame_ms"], 4)
    if "refit" in line:
        gain = line["refit"]["frame_ms"] - line["device_built"]["frame_ms"]
        line["breakeven_frames"] = round(rebuild_ms / gain, 2) if gain > 0 else None
        line["rebuild_ms"] = rebuild_ms
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cubes", action="store_true")
    a = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    scene, camera = read_file(DEFAULT_SCENE)
    cam = camera.convert_to_taichi_camera().packed()
    cornell = flatten_scene(scene)
    spins = S.spun(scene, 5, 6.0, 9)
    soup20k = soup(cornell, 20000, 9)
    t_cornell = time_rebuild("cornell", cornell, flatten_scene(spins[1]), 9)
    emit(t_cornell)
    t_soup = time_rebuild("soup-20000", soup20k, displaced(soup20k, 0.1, cornell.n_tri), 5)
    emit(t_soup)
    default = 0      # the scene's own kernel
    emit(quality_line("cornell", cornell, cornell, cam, default, t_cornell["rebuild_ms"]))
    emit(quality_line("cornell spin 48 deg", cornell, flatten_scene(spins[8]), cam, default, t_cornell["rebuild_ms"]))
    emit(quality_line("soup-20000", soup20k, soup20k, cam, 3, t_soup["rebuild_ms"]))
    for e in (0.1, 0.5, 1.0):
        emit(quality_line(f"soup-20000 third displaced {e} extent", soup20k, displaced(soup20k, e, cornell.n_tri), cam, 3,
                          t_soup["rebuild_ms"]))
    if not a.skip_cubes:
        cscene, ccamera = S.instanced_cubes()
        cubes = flatten_scene(cscene)
        t_cubes = time_rebuild("instanced_cubes", cubes, displaced(cubes, 0.01), 3)
        emit(t_cubes)
        emit(quality_line("instanced_cubes", cubes, cubes, ccamera.convert_to_taichi_camera().packed(), 3,
                          t_cubes["rebuild_ms"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(d) + "\n" for d in lines)


if __name__ == "__main__":
    main()

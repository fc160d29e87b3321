"""Measurements of the device refit against the only path there was before it, a new
DeviceScene per pose: JSON lines on stdout, kept in profiles/refit/.

    python tools/refit_time.py [--out profiles/refit/refit_time.jsonl] [--skip-cubes]

  update     per scene (Cornell, Cornell + a 20 000-triangle soup, instanced_cubes()): wall time of
             DeviceScene.update() and its split (host checks and packing, uploads, triangle records, tree levels,
             quantiser: prt_scene_download's PRT_BUF_UPDATE_MS, the kernel groups by HIP events), against
             DeviceScene(flat) + close() in the same process; `faster` says whether update() won
  sequence   wall time of `--frames 8 --spin 5 6 --resolution 128 128 --samples 1` with and without --refit
  tree       how a refit tree degrades: the Cornell short box spun in 6-degree steps, and a third of the soup's
             triangles displaced by 0.1, 0.5 and 1 scene extent; tree_cost() against its value at creation, and
             BVH node visits per query (the STATS words) of the refit scene against a rebuilt one
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
from pyrenderer_amd.flatten import FlatScene, flatten_scene  # noqa: E402
from pyrenderer_amd.io_utils.read_tungsten import read_file  # noqa: E402
from pyrenderer_amd.main import DEFAULT_SCENE, main as cli  # noqa: E402

F = np.float32


def with_vertices(f, tri_v):
    return FlatScene(tri_v, f.tri_n, f.tri_mat, f.tri_prim, f.prim_lo, f.prim_hi, f.mat, f.light_tri, f.light_off,
                     f.direct_rgb, f.sph, f.sph_mat, f.sph_prim)


def soup(f, n_extra, seed):
    """The Cornell box `f` plus n_extra small random triangles inside it (in front: the light's ids move)."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-0.9, 0.9, n_extra), rng.uniform(0.05, 1.8, n_extra), rng.uniform(-0.9, 0.9, n_extra)], 1)
    tv = (c[:, None, :] + rng.normal(0, 0.03, (n_extra, 3, 3))).astype(F).reshape(-1, 9)
    nn = np.cross((tv[:, 3:6] - tv[:, 0:3]).astype(np.float64), (tv[:, 6:9] - tv[:, 0:3]).astype(np.float64))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(F)
    lo = np.concatenate([tv.reshape(-1, 3).min(0)[None], f.prim_lo])
    hi = np.concatenate([tv.reshape(-1, 3).max(0)[None], f.prim_hi])
    return FlatScene(np.concatenate([tv, f.tri_v]), np.concatenate([nn, f.tri_n]),
                     np.concatenate([np.zeros(n_extra, np.int32), f.tri_mat]),
                     np.concatenate([np.zeros(n_extra, np.int32), f.tri_prim + 1]), lo, hi, f.mat,
                     f.light_tri + n_extra, f.light_off, f.direct_rgb)


def displaced(f, extents, skip_last=0):
    """Every third triangle (but the last skip_last, the room) moved along x by `extents` scene extents."""
    v = f.tri_v.copy().reshape(-1, 3, 3)
    p = v.reshape(-1, 3)
    n = v.shape[0] - skip_last
    v[:n:3, :, 0] += F(extents) * F((p.max(0) - p.min(0)).max())
    return with_vertices(f, v.reshape(-1, 9))


def time_update(name, flat, moved, reps):
    create = []
    for _ in range(reps):
        t0 = time.perf_counter()
        DeviceScene(moved, 0).close()
        create.append(time.perf_counter() - t0)
    ds = DeviceScene(flat, 0)
    ds.update(moved)                     # the first update allocates its device copies: not timed
    upd, split = [], []
    for k in range(reps):
        target = flat if k % 2 == 0 else moved
        t0 = time.perf_counter()
        ds.update(target)
        upd.append(time.perf_counter() - t0)
        split.append(ds.download("update_ms")[0])
    ds.close()
    s = np.median(np.array(split), axis=0)
    c, u = 1e3 * float(np.median(create)), 1e3 * float(np.median(upd))
    return dict(kind="update", scene=name, triangles=int(flat.n_tri), reps=reps, create_close_ms=round(c, 3),
                update_ms=round(u, 3), ratio=round(c / u, 2), faster=bool(u < c),
                split_ms=dict(host_pack=round(float(s[0]), 3), upload=round(float(s[1]), 3),
                              tri_records=round(float(s[2]), 3), tree_levels=round(float(s[3]), 3),
                              quantise=round(float(s[4]), 3)))


def visits_per_query(ds, cam, W, spp, depth):
    ids = interleaved_tiles(W, W, 64)
    ds.render_tiles(cam, W, W, 64, 64, ids, spp, depth, 1, N.PRT_FLAG_STATS)
    w = ds.diag_words(N.PRT_DIAG_WORDS)
    return float(w[N.PRT_DIAG_NODES]) / max(1.0, float(w[N.PRT_DIAG_EXT]) + float(w[N.PRT_DIAG_SHADOW]))


def tree_line(label, ds, cost0, flat, cam):
    ds.update(flat)
    fresh = DeviceScene(flat, 0)
    a, b = visits_per_query(ds, cam, 256, 4, 4), visits_per_query(fresh, cam, 256, 4, 4)
    line = dict(kind="tree", case=label, tree_cost_ratio=round(ds.tree_cost() / cost0, 4),
                rebuilt_cost_ratio=round(fresh.tree_cost() / cost0, 4), visits_per_query_refit=round(a, 3),
                visits_per_query_rebuilt=round(b, 3), visits_ratio=round(a / b, 4))
    fresh.close()
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
    emit(time_update("cornell", cornell, flatten_scene(spins[1]), 9))
    emit(time_update("soup-20000", soup20k, displaced(soup20k, 0.1, cornell.n_tri), 5))
    if not a.skip_cubes:
        cubes = flatten_scene(S.instanced_cubes()[0])
        emit(time_update("instanced_cubes", cubes, displaced(cubes, 0.01), 3))
        del cubes

    for flag in ([], ["--refit"]):
        argv = [DEFAULT_SCENE, "--samples", "1", "--depth", "4", "--resolution", "128", "128", "--frames", "8", "--spin",
                "5", "6", "--out", ""] + flag
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            cli(argv)
            walls.append(time.perf_counter() - t0)
        emit(dict(kind="sequence", refit=bool(flag), frames=8, wall_s=round(float(np.median(walls)), 4),
                  walls_s=[round(w, 4) for w in walls]))

    ds = DeviceScene(cornell, 0)
    cost0 = ds.tree_cost()
    for k in (1, 2, 4, 8):
        emit(tree_line(f"cornell spin {6 * k} deg", ds, cost0, flatten_scene(spins[k]), cam))
    ds.close()
    ds = DeviceScene(soup20k, 0)
    cost0 = ds.tree_cost()
    for e in (0.1, 0.5, 1.0):
        emit(tree_line(f"soup-20000 third displaced {e} extent", ds, cost0, displaced(soup20k, e, cornell.n_tri), cam))
    ds.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(d) + "\n" for d in lines)


if __name__ == "__main__":
    main()

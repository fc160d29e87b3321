"""What the parity tests share: the rays, the scenes used by more than one file, the caches of device
scenes and of oracle answers, and the comparisons themselves (closest and any-hit, traced paths, the
production / STATS render pair).  One copy of each; the test modules and the case modules (hard_scenes,
hard_spheres, shade_cases, global_cases, bvh8_scenes) import from here and never from each other's tests.

This is a plain module, not a conftest: pytest does not rewrite its assertions, so every `assert` here
carries the values it compared.  It imports numpy and the oracle, and pyrenderer_amd only inside the
functions that need it.

scene_cache comes in two forms: the generator, for a fixture that is `make` itself, and open_scenes, the
same generator as a context manager, only because a fixture that wraps `make` in a lambda cannot use
`yield from`.
"""
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import CORNELL_JSON
from oracle import oracle as O

MEDIA = os.path.dirname(CORNELL_JSON)

T_MIN, T_MAX = np.float32(1e-5), np.float32(99999.9)
ALL_VARIANTS = [1, 2, 3, 6, 7, 8, 4, 5]     # the parametrize order fixes the test ids


# ------------------------------------------------------------------ rays and range
def rays(n, seed, lo=(-1.0, 0.0, -1.0), hi=(1.0, 2.0, 1.0)):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def axis_rays(n, seed, lo=(-1.0, 0.0, -1.0), hi=(1.0, 2.0, 1.0)):
    """Directions with exact zero components (axis-parallel and diagonal-in-plane),
    and -0.0 as well as +0.0."""
    rng = np.random.default_rng(seed)
    dirs = []
    s = np.float32(np.sqrt(np.float32(0.5)))
    for a in range(3):
        for sign in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[a] = sign
            dirs.append(v)
            w = [-0.0, -0.0, -0.0]
            w[a] = sign
            dirs.append(w)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[a], v[b] = sa * s, sb * s
                dirs.append(v)
    dirs = np.array(dirs, np.float32)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    # some origins exactly on box-plane coordinates of the scene (walls at +-1, 0, 2)
    o[: n // 4, 0] = rng.choice(np.array([-1.0, 1.0, 0.0, 0.5], np.float32), n // 4)
    oo = np.repeat(o, len(dirs), axis=0)
    dd = np.tile(dirs, (n, 1))
    return oo, dd


def random_bounds(osc, o, d, seed):
    """Shadow-style t_max per ray: around the ray's own closest hit (0.5 .. 1.5 of it), so about half
    the queries are occluded wherever the scene sits; rays without a hit get T_MAX."""
    hit, t, _, _ = osc.closest(o, d, T_MIN, T_MAX)
    k = np.random.default_rng(seed).uniform(0.5, 1.5, o.shape[0])
    return np.where(hit != 0, t.astype(np.float64) * k, float(T_MAX)).astype(np.float32)


# ------------------------------------------------------------------ scenes used across files
def soup_scene(cornell, n_extra, seed):
    """Cornell + a random triangle soup inside the box (config 4's shape, small)."""
    from pyrenderer_amd.flatten import FlatScene
    f = cornell[2]
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-0.9, 0.9, n_extra), rng.uniform(0.05, 1.8, n_extra), rng.uniform(-0.9, 0.9, n_extra)], 1)
    tv = (c[:, None, :] + rng.normal(0, 0.03, (n_extra, 3, 3))).astype(np.float32).reshape(-1, 9)
    e1 = tv[:, 3:6] - tv[:, 0:3]
    e2 = tv[:, 6:9] - tv[:, 0:3]
    nn = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)
    # extra triangles first so the light's triangle ids move
    tri_v = np.concatenate([tv, f.tri_v])
    tri_n = np.concatenate([nn, f.tri_n])
    tri_mat = np.concatenate([np.full(n_extra, 0, np.int32), f.tri_mat])
    tri_prim = np.concatenate([np.zeros(n_extra, np.int32), f.tri_prim + 1])
    lo = np.concatenate([tv.reshape(-1, 3, 3).min(1).min(0)[None], f.prim_lo])
    hi = np.concatenate([tv.reshape(-1, 3, 3).max(1).max(0)[None], f.prim_hi])
    return FlatScene(tri_v, tri_n, tri_mat, tri_prim, lo, hi, f.mat, f.light_tri + n_extra, f.light_off, f.direct_rgb)


def specular_scene(rough=0.0, spheres=True):
    """(scene, camera, flat) of the specular Cornell box with the metal's roughness set."""
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.io_utils.read_tungsten import process_primitives
    d = json.load(open(os.path.join(MEDIA, "scene_specular.json")))
    for b in d["bsdfs"]:
        if b["type"] == "metal":
            b["roughness"] = rough
    if not spheres:
        d["primitives"] = [p for p in d["primitives"] if p["type"] != "sphere"]
    scene, cam = process_primitives(d)
    return scene, cam, flatten_scene(scene)


def scene_json(tmp_path):
    """The Cornell box's Tungsten JSON with a second light quad and an emitting cube, written to tmp_path."""
    import copy
    d = json.load(open(CORNELL_JSON))
    lights = [p for p in d["primitives"] if p.get("bsdf") == "Light"]
    q = copy.deepcopy(lights[0])
    q["transform"]["position"] = [0.45, 1.6, 0.2]          # a second, lower light quad
    c = {"transform": {"position": [-0.6, 1.7, 0.5], "scale": [0.1, 0.1, 0.1], "rotation": [0, 30, 0]},
         "type": "cube", "bsdf": "Light"}                 # and an emitting cube (12 faces)
    d["primitives"] += [q, c]
    p = tmp_path / "scene.json"
    p.write_text(json.dumps(d))
    return str(p)


def fnv1a64(a):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


# ------------------------------------------------------------------ small helpers
def packed_camera(cornell):
    return cornell[1].convert_to_taichi_camera().packed()


def all_tiles(W, H, tile):
    """The ids of every tile of a W x H frame, in order."""
    return np.arange(((W + tile - 1) // tile) * ((H + tile - 1) // tile), dtype=np.int32)


def is_mis(v):
    """Variant `v` is one of the MIS estimator's: its reference is the oracle's under nee_mode(True)."""
    from pyrenderer_amd import _native as N
    return v in N.VAR_MIS


def variant_flags(v):
    """The launch flags that force trace-kernel variant `v` (with the MIS estimator where `v` is one of its)."""
    from pyrenderer_amd import _native as N
    return (v << 8) | (N.PRT_FLAG_MIS_NEE if is_mis(v) else 0)


# ------------------------------------------------------------------ comparisons
def wrong_rows(got, want, nan_aware=False):
    """Row indices on which `got` differs from `want`: as uint32 bits, or NaN-aware: a NaN wherever the
    other has one, and the same bits everywhere else."""
    same = got.view(np.uint32) == want.view(np.uint32)
    if nan_aware:
        same |= np.isnan(got) & np.isnan(want)
    return np.nonzero(~same.reshape(same.shape[0], -1).all(axis=1))[0]


def hit_ids(hit, tri):
    """The oracle's (hit flag, primitive) as prt_closest_hits' ids: -1 on a miss."""
    return np.where(hit != 0, tri, -1).astype(np.int64)


def hits_wrong(ds, osc, o, d, tmin, tmax, quantized, any_hit, want=None):
    """One comparison of prt_closest_hits with brute force: (count, first three offenders with both
    answers, oracle hit mask).  Closest: (id, t) must be equal, offenders are (i, o, d, id, oracle id, t,
    oracle t).  Any-hit: hit or miss must be equal, offenders are (i, o, d, t_max, id, oracle hit).  `want` is
    the oracle's answer where the caller has it already: (ids, t), or the hit mask for any-hit."""
    if want is None:
        hit, ot, tri, _ = osc.closest(o, d, tmin, tmax)
        want = hit != 0 if any_hit else (hit_ids(hit, tri), ot)
    gid, gt = ds.closest_hits(o, d, tmin, tmax, any_hit=any_hit, quantized=quantized)
    if any_hit:
        bad = np.nonzero((gid >= 0) != want)[0]
        tm = np.broadcast_to(tmax, want.shape)
        return bad.size, [(i, o[i], d[i], tm[i], gid[i], want[i]) for i in bad[:3]], want
    oid, ot = want
    bad = np.nonzero((gid != oid) | ((gid >= 0) & (gt != ot)))[0]
    return bad.size, [(i, o[i], d[i], gid[i], oid[i], gt[i], ot[i]) for i in bad[:3]], oid >= 0


def check_trace(ds, ref, o, d, depth, seed, v, *, label, lds_scene=None, width=None, expect=None, finite=True,
                ties=None):
    """`o`, `d` through prt_trace_rays in forced variant `v` against the oracle's `ref`, bit for bit.
    First the launch has to be the one under test: kernel_info() names variant `v` and, where given, the
    scene's LDS residency, the tree `width` of an LDS kernel and the further `expect` items; and the reference has to be
    what the case is for: finite and not black, or with `finite=False` non-finite on at least one and at
    most half of the rays, which are then compared NaN for NaN.  `ties` marks the rays whose hit is a tie,
    for the message."""
    n = o.shape[0]
    flags = variant_flags(v)
    if lds_scene is not None:
        assert ds.kernel_info()["lds_scene"] == lds_scene, (label, lds_scene, ds.kernel_info())
    info = ds.kernel_info(n_items=n, flags=flags)
    assert info["variant"] == v, (label, v, info)
    if width is not None:
        assert info["bvh_arity"] == width and info["lds_scene"], (label, v, width, info)
    for k, want in (expect or {}).items():
        assert info[k] == want, (label, v, k, want, info)
    bad_ref = int((~np.isfinite(ref)).any(axis=1).sum())
    if finite:
        assert bad_ref == 0 and ref.mean() > 0, (label, bad_ref, ref.mean())
    else:
        assert 1 <= bad_ref <= n // 2, (label, bad_ref, n)
    L = ds.trace_rays(o, d, depth, seed=seed, flags=flags)
    ds.check_faults()
    bad = wrong_rows(L, ref, nan_aware=not finite)
    print(f"{label}: variant {info['variant']} ran at bvh_arity {info['bvh_arity']}, stack {info['stack']}, {n} rays, "
          f"{bad.size} differ from the oracle")
    on_ties = None if ties is None else "%d of the differing rays are tie rays" % int(ties[bad].sum())
    assert bad.size == 0, (label, v, bad.size, on_ties, [(i, o[i], d[i], L[i], ref[i]) for i in bad[:3]])


def render_twice(ds, cam, W, H, tile, ids, spp, depth, seed, flags, *, width=None):
    """One launch in the production and in the STATS build: dict(img, queries = (extension, shadow) counts,
    words = the diag words, info = kernel_info of the launch).  Asserts no fault after either, no
    non-finite sample and the STATS image equal to the production one; that the launch takes the variant
    `flags` force, if they force one; with `width`, that an LDS kernel runs at that tree width and the
    deepest stack entry touched stays within the stack's size."""
    from pyrenderer_amd import _native as N
    info = ds.kernel_info(len(ids) * tile * tile * spp, flags)
    forced = (flags >> 8) & 0xFF
    assert not forced or info["variant"] == forced, (forced, info)
    if width is not None:
        assert info["bvh_arity"] == width and info["lds_scene"], (width, info)
    img, _ = ds.render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed, flags)
    ds.check_faults()
    simg, st = ds.render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed, flags | N.PRT_FLAG_STATS)
    ds.check_faults()
    w = ds.diag_words(N.PRT_DIAG_WORDS)
    assert int(w[N.PRT_DIAG_NONFINITE]) == 0, (int(w[N.PRT_DIAG_NONFINITE]), info)
    if width is not None:
        assert 1 <= int(w[N.PRT_DIAG_MAX_STACK]) <= info["stack"], (int(w[N.PRT_DIAG_MAX_STACK]), info)
    differ = int((simg != img).any(axis=-1).sum())
    assert differ == 0, ("STATS image differs from the production one", differ, info)
    return dict(img=img, queries=(int(st[2]), int(st[3])), words=w, info=info)


# ------------------------------------------------------------------ environment knobs and device scenes
@contextmanager
def env_knobs(**knobs):
    """The environment with each knob set to str(value), or unset where the value is None; restored on
    exit, however it exits.  Scenes and trees read their knobs when they are created."""
    old = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def scene_cache():
    """For `yield from` in a module-scoped fixture: yields make(key, flat_or_factory, **knobs), which
    creates the DeviceScene of `flat` (or calls the factory) once per (key, knobs) under env_knobs(**knobs),
    and closes every scene it made at teardown."""
    made = {}

    def make(key, flat_or_factory, **knobs):
        k = (key, tuple(sorted(knobs.items())))
        if k not in made:
            with env_knobs(**knobs):
                if callable(flat_or_factory):
                    made[k] = flat_or_factory()
                else:
                    from pyrenderer_amd.device_scene import DeviceScene
                    made[k] = DeviceScene(flat_or_factory, 0)
        return made[k]
    try:
        yield make
    finally:
        for ds in made.values():
            ds.close()


# scene_cache as a context manager: a fixture that hands out a wrapper of `make` (other arguments, a fixed
# knob) has to yield that wrapper itself and so cannot `yield from scene_cache()`
open_scenes = contextmanager(scene_cache)


def world_cache(case):
    """For `yield from` in a module-scoped `world` fixture: yields get(name) -> (DeviceScene, OracleScene,
    whatever else case(name) returns after its FlatScene); each scene is created once."""
    oracles = {}

    def get(name):
        flat, *rest = case(name)
        if name not in oracles:
            oracles[name] = O.OracleScene.from_flat(flat)
        return (make(name, flat), oracles[name], *rest)
    with open_scenes() as make:
        yield get


@pytest.fixture(scope="module")
def scenes_by_width():
    """make(name, flat, width, **env) -> DeviceScene created with PRT_LDS_WIDTH = width (None: unset) and
    the other knobs given (cached)."""
    with open_scenes() as make:
        yield lambda name, flat, width, **env: make(name, flat, PRT_LDS_WIDTH=width, **env)


# ------------------------------------------------------------------ oracle answers
@contextmanager
def nee_mode(mis):
    """The oracle's direct-lighting estimator: the reference's (False) or the MIS one (True) inside the
    block, the reference's again after it, however it exits."""
    O.set_nee_mode(mis)
    try:
        yield
    finally:
        O.set_nee_mode(False)


class OracleRefs:
    """The cache of one module's oracle answers, keyed by the tuple the caller gives."""

    def __init__(self):
        self._made = {}

    def get(self, key, compute):
        if key not in self._made:
            self._made[key] = compute()
        return self._made[key]

    def trace(self, key, osc, o, d, depth, seed, mis, nthreads=None):
        """osc.trace_rays under the reference estimator or (mis) the MIS one."""
        def compute():
            with nee_mode(mis):
                return osc.trace_rays(o, d, depth, seed=seed, nthreads=nthreads or 0)
        return self.get(("trace", key, mis), compute)

    def render_tiles(self, key, osc, cam, W, H, tile, ids, spp, depth, seed, mis=False, nthreads=None):
        """(slot sums, (extension, shadow) query counts) of osc.render_tiles(..., counters=True)."""
        def compute():
            with nee_mode(mis):
                ref, cnt = osc.render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed=seed, nthreads=nthreads or 0,
                                            counters=True)
            return ref, (int(cnt[2]), int(cnt[3]))
        return self.get(("render", key, mis), compute)

    def closest(self, key, osc, o, d, tmin=T_MIN, tmax=T_MAX):
        """Brute-force (ids, t) of one ray set."""
        def compute():
            hit, t, tri, _ = osc.closest(o, d, tmin, tmax)
            return hit_ids(hit, tri), t
        return self.get(("closest", key), compute)

"""Hit-level GPU parity: `prt_closest_hits` (the kernels' BVH4 traversal, float and
quantised nodes, + spheres) against the oracle's brute-force `World.hit_all`
(mathematics/intersection_taichi.py:238-291) on the same rays, bit for bit.

Includes rays with direction components of exactly 0 (1/d = inf): the case where a
min/max slab formulation turns a NaN plane distance into a wrong cull.
"""
import numpy as np
import pytest

from kernel_parity import T_MAX, T_MIN, axis_rays, hits_wrong, rays, soup_scene, specular_scene
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _check_closest(ds, osc, o, d, quantized=False):
    n, first, ohit = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized, any_hit=False)
    assert n == 0, (n, first)
    return ohit.mean()


def _check_any(ds, osc, o, d, tmax, quantized=False):
    n, first, _ = hits_wrong(ds, osc, o, d, T_MIN, tmax, quantized, any_hit=True)
    assert n == 0, (n, first)


@pytest.mark.parametrize("quantized", [False, True])
def test_cornell_hits_match_oracle(gpu_scene, oracle_scene, quantized):
    o, d = rays(20000, 1)
    frac = _check_closest(gpu_scene, oracle_scene, o, d, quantized)
    assert frac > 0.5
    o, d = axis_rays(3000, 2)
    _check_closest(gpu_scene, oracle_scene, o, d, quantized)
    # shadow-style bounded queries
    o, d = rays(20000, 3)
    tmax = np.random.default_rng(4).uniform(0.01, 3.0, o.shape[0]).astype(np.float32)
    _check_any(gpu_scene, oracle_scene, o, d, tmax, quantized)


@pytest.mark.parametrize("quantized", [False, True])
def test_soup_hits_match_oracle(cornell, quantized):
    from pyrenderer_amd.device_scene import DeviceScene
    flat = soup_scene(cornell, 3000, 9)
    ds = DeviceScene(flat, 0)
    try:
        osc = O.OracleScene.from_flat(flat)
        o, d = rays(20000, 5)
        _check_closest(ds, osc, o, d, quantized)
        o, d = axis_rays(2000, 6)
        _check_closest(ds, osc, o, d, quantized)
    finally:
        ds.close()


def test_sphere_scene_hits_match_oracle():
    from pyrenderer_amd.device_scene import DeviceScene
    _, _, flat = specular_scene(0.0)
    ds = DeviceScene(flat, 0)
    try:
        osc = O.OracleScene.from_flat(flat)
        o, d = rays(20000, 7)
        _check_closest(ds, osc, o, d)
        o, d = axis_rays(1000, 8)
        _check_closest(ds, osc, o, d)
    finally:
        ds.close()

"""The scenes of tests/shade_cases.py against the host's classification and the oracle alone (no GPU):
the inputs contain what they are built for, so tests/test_gpu_shade_cases.py cannot pass vacuously.

The host side goes through the stand-alone driver of tests/host_plan_driver.py (pack_scene in its
sanitizer build): each case's (plain, shade_fast) is what the table says.  The oracle side traces the
4096 rays at depth 8 with seed 17 under both direct-lighting estimators: the finite cases stay finite and
carry light, the overflow cases overflow on a few paths, and on every case at least 1000 paths differ in
bits from the unedited scene's, so the edited rows and normals are reached.

Measured with the brute-force backend, reference estimator / MIS, paths that differ from the unedited
scene: black 1501 / 1655, red 1251 / 1424, tiny, denormal, below and lo-edge 1065 / 1203, red-light
2593 / 2892, n3 2247 / 2569, n-quarter 2188 / 2545, n2-over 2179 / 2535, n2 2172 / 2532, n-half
2179 / 2535, above and hi-edge 1065 / 1206, soup-black 2309 / 2609.  Non-finite rows: above and hi-edge 3 / 76
(6 of the 76 hold a NaN), every other case 0 / 0; hi-edge needed no deeper paths than above.
"""
import numpy as np
import pytest

import shade_cases as C
from host_plan_driver import _flat_args, _scene, built  # noqa: F401  (built: the driver's fixture)
from kernel_parity import OracleRefs, nee_mode, wrong_rows
from oracle import oracle as O

F = np.float32
REFS = OracleRefs()


def _trace(cornell, name, mis, edited=True):
    """The oracle's radiance of the case's rays, (4096, 3); of the unedited scene with edited=False."""
    key = name if edited else "base-" + ("soup" if name == C.SOUP else "box")
    def compute():
        flat = C.case(cornell, name) if edited else C.base(cornell, name)
        with nee_mode(mis):
            return O.OracleScene.from_flat(flat).trace_rays(*C.rays(), C.DEPTH, seed=C.SEED)
    return REFS.get((key, mis), compute)


def _differ(cornell, name, mis):
    return wrong_rows(_trace(cornell, name, mis), _trace(cornell, name, mis, False)).size


def test_rows_are_the_walls_they_are_named_for(cornell):
    flat = cornell[2]
    v = flat.tri_v.reshape(-1, 3, 3)
    for row, axis, at in ((C.FLOOR, 1, 0.0), (C.BACK, 2, -1.0), (C.RED_WALL, 0, -1.0)):
        t = flat.tri_mat == row
        assert t.sum() == 2 and (v[t][..., axis] == F(at)).all() and flat.mat[row, 3] == 0, row
    assert np.array_equal(np.nonzero(flat.tri_mat == C.LIGHT)[0], np.sort(flat.light_tri)) and flat.mat[C.LIGHT, 3] > 0
    assert flat.mat[C.RED_WALL, 0] > 4 * flat.mat[C.RED_WALL, 1]
    o, d = C.rays()
    assert o.shape == d.shape == (C.N_RAYS, 3) and o.dtype == d.dtype == F


def test_bounds_and_values_are_the_f32_numbers_they_claim():
    assert C.LO == F(2.0) ** -40 and C.HI == F(2.0) ** 40 and float(C.LO) == 2.0 ** -40 and float(C.HI) == 2.0 ** 40
    below = np.nextafter(C.LO, F(0))
    assert below.dtype == F and below < C.LO and np.nextafter(below, F(1)) == C.LO
    tiny = np.finfo(F).tiny
    assert 0 < F(1e-40) < tiny and F(1e-20) > tiny                       # a denormal, and a normal one
    assert F(2.0 ** 41) > C.HI


@pytest.mark.parametrize("name", C.CASES)
def test_only_the_named_table_is_replaced(cornell, name):
    """mat or tri_n differs from the unedited scene, in the entries the case names and nowhere else."""
    b, flat = C.base(cornell, name), C.case(cornell, name)
    for field in ("tri_v", "tri_mat", "tri_prim", "prim_lo", "prim_hi", "light_tri", "light_off"):
        assert np.array_equal(getattr(flat, field), getattr(b, field)), field
    assert flat.sph.shape[0] == 0 and flat.mat.dtype == F and flat.tri_n.dtype == F
    assert flat.mat.shape == b.mat.shape and flat.tri_n.shape == b.tri_n.shape and flat.n_light == b.n_light
    assert np.array_equal(flat.direct_rgb, b.direct_rgb)
    dm = np.argwhere(flat.mat.view(np.uint32) != b.mat.view(np.uint32))
    dn = np.unique(np.argwhere(flat.tri_n.view(np.uint32) != b.tri_n.view(np.uint32))[:, 0])
    ch = [C.FLOOR, C.CHANNEL]
    want_mat = {"black": [[C.BACK, c] for c in range(3)], "red": [[C.RED_WALL, c] for c in range(3)],
                "red-light": [[C.LIGHT, 1], [C.LIGHT, 2]], C.SOUP: [[C.BACK, c] for c in range(3)]}
    want_mat.update({k: [ch] for k in ("tiny", "denormal", "below", "above", "lo-edge", "hi-edge")})
    assert dm.tolist() == want_mat.get(name, []), (name, dm)
    value = {"tiny": F(1e-20), "denormal": F(1e-40), "below": np.nextafter(C.LO, F(0)), "above": F(2.0 ** 41),
             "lo-edge": C.LO, "hi-edge": C.HI}
    if name in value:
        assert flat.mat[C.FLOOR, C.CHANNEL] == value[name] and flat.mat[C.FLOOR, C.CHANNEL] > 0
    if name in ("black", C.SOUP):
        assert not flat.mat[C.BACK, :3].any()
    if name in ("red", "red-light"):
        assert flat.mat[C.RED_WALL if name == "red" else C.LIGHT, :3].tolist() == [1, 0, 0]
    # the normals: which triangles, and their exact squared lengths as the host measures them
    every, scale = {"n3": (3, 3), "n2-over": (3, 2), "n2": (3, 2), "n-half": (3, 0.5), "n-quarter": (5, 0.25),
                    C.SOUP: (3, 3)}.get(name, (0, 1))
    ids = C.scaled_triangles(b, every) if every else np.zeros(0, np.int64)
    if name == "n2":
        ids = ids[C.exactly_unit(b)[ids]]
    assert np.array_equal(dn, ids), (name, dn)
    if every:
        lights, walls = np.isin(ids, b.light_tri), np.isin(b.tri_mat[ids], [C.FLOOR, 1, C.BACK, 3, C.RED_WALL])
        if name == C.SOUP:
            walls &= ids >= 300                                           # the soup's triangles share the floor's row
        assert lights.any() and walls.any(), (name, ids)
        assert (~C.exactly_unit(b)[ids]).any() == (name != "n2")          # the rotated boxes' faces are among them
        n = flat.tri_n.astype(np.float64)
        l2 = (n * n).sum(1)
        assert (l2[ids] == scale * scale).any() and np.abs(l2[ids] / (scale * scale) - 1).max() < 1e-6
        if scale != 3:                                                    # a power of two: exact
            assert np.array_equal(flat.tri_n[ids], b.tri_n[ids] * F(scale))
            assert np.array_equal(l2[ids], scale * scale * (b.tri_n[ids].astype(np.float64) ** 2).sum(1))
        inside = bool(((l2 >= 0.25) & (l2 <= 4.0)).all())
        assert inside == (name in ("n2", "n-half")), (name, l2.min(), l2.max())
        if name == "n2":
            assert l2.max() == 4.0
        if name == "n-half":
            assert l2.min() == 0.25
        if name == "n2-over":
            assert 4.0 < l2.max() < 4.000001


@pytest.mark.parametrize("name", C.CASES)
def test_host_classification_equals_the_table(built, tmp_path, cornell, name):  # noqa: F811
    rep = _scene(built, str(tmp_path), _flat_args(C.case(cornell, name)))
    _, plain, shade_fast, _ = C.TABLE[name]
    assert rep["error"] is None and (rep["plain"], rep["shade_fast"]) == (plain, shade_fast), (name, rep)


def test_unedited_scenes_keep_the_fast_guards(built, tmp_path, cornell):  # noqa: F811
    for k, name in enumerate(("black", C.SOUP)):
        rep = _scene(built, str(tmp_path / str(k)), _flat_args(C.base(cornell, name)))
        assert rep["error"] is None and rep["plain"] is True and rep["shade_fast"] is True


def test_the_table_covers_both_sides():
    assert set(C.TABLE) == set(C.CASES) and len(C.CASES) == 15 and sorted(C.OVERFLOW) == ["above", "hi-edge"]
    on = [k for k in C.CASES if C.TABLE[k][2]]
    assert sorted(on) == ["hi-edge", "lo-edge", "n-half", "n2"]
    assert all(C.TABLE[k][1] for k in C.CASES)                           # no sphere, metal or dielectric anywhere


def test_nan_aware_comparison_forgives_payloads_only():
    """The comparison tests/test_gpu_shade_cases.py uses on the overflow cases."""
    a = np.array([[1, np.inf, np.nan], [0, 2, 3]], F)
    b = a.copy()
    b.view(np.uint32)[0, 2] ^= 1                                        # another payload of the same NaN
    assert wrong_rows(a, b, True).size == 0 and wrong_rows(a, b, False).tolist() == [0]
    for edit in ((0, 1, -np.inf), (0, 2, np.inf), (1, 0, -0.0), (1, 1, np.nan)):
        c = b.copy()
        c[edit[:2]] = edit[2]
        assert wrong_rows(a, c, True).tolist() == [edit[0]], edit


@pytest.mark.parametrize("mis", [False, True], ids=["reference", "mis"])
@pytest.mark.parametrize("name", C.FINITE)
def test_finite_cases_stay_finite_and_reach_their_edits(cornell, name, mis):
    L = _trace(cornell, name, mis)
    n = _differ(cornell, name, mis)
    print("%s %s: mean %.6g, %d of %d paths differ from the unedited scene" % (name, "mis" if mis else "ref", L.mean(),
                                                                               n, C.N_RAYS))
    assert L.shape == (C.N_RAYS, 3) and np.isfinite(L).all() and L.mean() > 0, name
    assert n >= 1000, (name, n)


@pytest.mark.parametrize("mis", [False, True], ids=["reference", "mis"])
@pytest.mark.parametrize("name", C.OVERFLOW)
def test_overflow_cases_overflow_on_a_few_paths(cornell, name, mis):
    """Four visits to the floor multiply one channel of the throughput by 2^160 or 2^164: measured 3 rows
    with an infinity under the reference estimator, 76 non-finite rows (6 with a NaN) under MIS, for `above`
    and for `hi-edge` alike at depth 8."""
    L = _trace(cornell, name, mis)
    bad = int((~np.isfinite(L)).any(axis=1).sum())
    n = _differ(cornell, name, mis)
    print("%s %s: %d non-finite rows (%d with a NaN), %d paths differ" % (name, "mis" if mis else "ref", bad,
                                                                          int(np.isnan(L).any(axis=1).sum()), n))
    assert 1 <= bad <= C.N_RAYS // 2, (name, bad)
    assert n >= 1000, (name, n)
    assert np.isfinite(_trace(cornell, name, mis, False)).all()

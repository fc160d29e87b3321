"""Scene arguments that prt_scene_create rejects, with the message of the first check each one fails.
Shared by tests/test_scene_abi.py (through the C ABI) and tests/test_host_plan.py (through the
sanitizer build of the validation itself), so both see the same cases and texts."""
import numpy as np

F, I = np.float32, np.int32
ARRAYS = ("tri_v", "tri_n", "tri_mat", "sph", "sph_mat", "mat", "light_tri", "light_off")
COUNTS = ("n_tri", "n_sph", "n_mat", "n_light")


def base_scene():
    """One emitting triangle, one material, one light."""
    return dict(tri_v=np.array([[0, 0, 0, 1, 0, 0, 0, 0, 1]], F), tri_n=np.array([[0, 1, 0]], F),
                tri_mat=np.array([0], I), n_tri=1, sph=None, sph_mat=None, n_sph=0,
                mat=np.array([[0.5, 0.5, 0.5, 1, 0, 0, 1, 0]], F), n_mat=1,
                light_tri=np.array([0], I), light_off=np.array([0, 1], I), n_light=1)


def scene(**over):
    s = base_scene()
    s.update(over)
    return s


_TWO = dict(tri_v=np.tile(base_scene()["tri_v"], (2, 1)), tri_n=np.tile(base_scene()["tri_n"], (2, 1)), n_tri=2)
_SPH = dict(sph=np.array([[0, 0, 0, 1]], F), sph_mat=np.array([0], I), n_sph=1)

# (id, arguments, message); the last four violate two checks: the earlier one reports
REJECTED = [
    ("n_tri_negative", scene(n_tri=-1), "bad triangle arrays"),
    ("tri_v_null", scene(tri_v=None), "bad triangle arrays"),
    ("tri_n_null", scene(tri_n=None), "bad triangle arrays"),
    ("tri_mat_null", scene(tri_mat=None), "bad triangle arrays"),
    ("n_sph_negative", scene(n_sph=-1), "bad sphere arrays"),
    ("sph_null", scene(**dict(_SPH, sph=None)), "bad sphere arrays"),
    ("sph_mat_null", scene(**dict(_SPH, sph_mat=None)), "bad sphere arrays"),
    ("sph_mat_range", scene(**dict(_SPH, sph_mat=np.array([1], I))), "sphere material id out of range"),
    ("sph_mat_negative", scene(**dict(_SPH, sph_mat=np.array([-1], I))), "sphere material id out of range"),
    ("sph_radius_zero", scene(**dict(_SPH, sph=np.array([[0, 0, 0, 0]], F))), "sphere radius must be > 0"),
    ("sph_radius_nan", scene(**dict(_SPH, sph=np.array([[0, 0, 0, np.nan]], F))), "sphere radius must be > 0"),
    ("too_many_primitives", scene(n_tri=1 << 31), "too many primitives"),
    ("n_mat_zero", scene(n_mat=0), "need at least one material"),
    ("mat_null", scene(mat=None), "need at least one material"),
    ("n_light_zero", scene(n_light=0), "There is no lights!!! (n_light < 1)"),
    ("light_off_null", scene(light_off=None), "There is no lights!!! (n_light < 1)"),
    ("light_tri_null", scene(light_tri=None), "There is no lights!!! (n_light < 1)"),
    ("tri_mat_range", scene(**dict(_TWO, tri_mat=np.array([0, 5], I))), "material id out of range at triangle 1"),
    ("tri_mat_negative", scene(tri_mat=np.array([-1], I)), "material id out of range at triangle 0"),
    ("light_off_start", scene(light_off=np.array([1, 2], I)), "light_off[0] must be 0"),
    ("light_empty", scene(light_off=np.array([0, 0], I)), "every light needs >= 1 triangle"),
    ("light_tri_range", scene(light_tri=np.array([1], I)), "light triangle out of range"),
    ("light_tri_negative", scene(light_tri=np.array([-1], I)), "light triangle out of range"),
    ("first_tri_then_sph", scene(tri_v=None, n_sph=-1), "bad triangle arrays"),
    ("first_sph_then_mat", scene(n_mat=0, **dict(_SPH, sph=np.array([[0, 0, 0, -1]], F))),
     "sphere material id out of range"),
    ("first_mat_then_light", scene(n_mat=0, n_light=0), "need at least one material"),
    ("first_tri_mat_then_light_off", scene(tri_mat=np.array([3], I), light_off=np.array([1, 1], I)),
     "material id out of range at triangle 0"),
]

"""The PRT_FLAG_STATS counters of one render read back four ways — prt_render_tiles' own output,
prt_last_stats, prt_diag_stats and prt_diag_words — are the same four words (one read-back in
pyrenderer_amd/csrc/prt_capi.cpp serves all of them)."""
import numpy as np
import pytest

from pyrenderer_amd._native import PRT_FLAG_STATS

pytestmark = pytest.mark.gpu


def test_stats_read_back_paths_agree(gpu_scene, cornell):
    cam = cornell[1].convert_to_taichi_camera().packed()
    W = H = 8
    ids = np.zeros(1, np.int32)   # the frame is one 8 x 8 tile
    _, st = gpu_scene.render_tiles(cam, W, H, 8, 8, ids, 1, 2, seed=1, flags=PRT_FLAG_STATS)
    paths = {"render_tiles": st, "last_stats": gpu_scene.last_stats(), "diag_stats": gpu_scene.diag_stats()[:4],
             "diag_words": gpu_scene.diag_words(4)}
    print({k: v.tolist() for k, v in paths.items()})
    assert st.shape == (4,) and (st != 0).all()   # nodes, triangles, extension and shadow queries
    for name, v in paths.items():
        assert np.array_equal(v, st), name
    # more words than the library keeps read as zeros past the end
    wide = gpu_scene.diag_words(200)
    assert np.array_equal(wide[:4], st) and not wide[192:].any()
    _, plain = gpu_scene.render_tiles(cam, W, H, 8, 8, ids, 1, 2, seed=1)
    assert not plain.any()
    gpu_scene.check_faults()

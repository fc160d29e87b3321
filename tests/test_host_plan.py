"""The host arithmetic of libprt that needs no GPU (pyrenderer_amd/csrc/prt_plan.cpp: scene checks and
packing, environment knobs, tile / window / ownership arithmetic, the launch-chunk plan, camera terms),
run in its AddressSanitizer + UndefinedBehaviorSanitizer build through the stand-alone driver
tools/sanitize/host_check.cpp and compared with numpy restatements.  A subprocess per call: exit code 0,
no sanitizer text on stderr, one JSON line on stdout."""
import os

import numpy as np
import pytest

from host_plan_driver import _flat_args, _run, _scene, built  # noqa: F401  (built: the driver's fixture)
from scene_cases import REJECTED, base_scene, scene

F = np.float32


# ---------------------------------------------------------------- tiles, windows, ownership

@pytest.mark.parametrize("tw,th", [(8, 8), (16, 4)])
def test_tile_origins_decode_to_the_tile_corner(built, tw, th):
    W, H = 100, 70   # the ragged frame of test_gpu_boundary
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    ids = list(range(tiles_x * tiles_y)) + [-1]
    xy = _run(built, "origins", tiles_x, tw, th, *ids)["origins"]
    assert len(xy) == len(ids)
    for i, v in zip(ids[:-1], xy[:-1]):
        assert (v >> 16, v & 0xFFFF) == ((i % tiles_x) * tw, (i // tiles_x) * th)
    assert xy[-1] == 0xFFFF0000


@pytest.mark.parametrize("win", [(0, 0, 100, 70), (37, 41, 1, 1), (8, 16, 24, 16)],
                         ids=["full_frame", "one_pixel", "ends_on_tile_edge"])
def test_window_tiles_cover_the_window_and_only_touched_tiles(built, win):
    W, H, tw, th = 100, 70, 8, 8
    x0, y0, w, h = win
    ids = _run(built, "window", W, x0, y0, w, h, tw, th)["ids"]
    tiles_x = -(-W // tw)
    ty, tx = np.meshgrid(np.arange(y0 // th, (y0 + h - 1) // th + 1), np.arange(x0 // tw, (x0 + w - 1) // tw + 1),
                         indexing="ij")
    assert ids == (ty * tiles_x + tx).ravel().tolist()
    covered = np.zeros((W + tw, H + th), bool)
    for i in ids:
        cx, cy = (i % tiles_x) * tw, (i // tiles_x) * th
        # every tile touches the window ...
        assert cx < x0 + w and cx + tw > x0 and cy < y0 + h and cy + th > y0
        covered[cx:cx + tw, cy:cy + th] = True
    # ... and together they cover it
    assert covered[x0:x0 + w, y0:y0 + h].all()


def test_slots_outside_a_ragged_frame_are_flagged(built):
    W, H, tw, th = 100, 70, 8, 8
    tiles_x = -(-W // tw)
    ids = [0, tiles_x - 1, tiles_x * 8, tiles_x * 9 - 1]   # inner, right edge, bottom edge, corner
    got = np.array(_run(built, "in_frame", W, H, tw, th, *ids)["in_frame"]).reshape(len(ids), th, tw)
    for k, i in enumerate(ids):
        x = (i % tiles_x) * tw + np.arange(tw)[None, :]
        y = (i // tiles_x) * th + np.arange(th)[:, None]
        assert np.array_equal(got[k].astype(bool), (x < W) & (y < H))
    assert got[0].all() and not got[3].all()


def test_latin_stride_matches_the_python_owner(built):
    from pyrenderer_amd.device_scene import latin_stride
    assert _run(built, "latin_stride", 1, 64)["strides"] == [latin_stride(n) for n in range(1, 65)]


@pytest.mark.parametrize("W,H,tile", [(128, 128, 16), (100, 70, 8)])
def test_per_rank_tile_lists_match_tile_owner(built, W, H, tile):
    from pyrenderer_amd.device_scene import tile_owner
    for n in (1, 2, 3, 5, 8):
        owner = tile_owner(W, H, tile, n, "latin")
        ids = _run(built, "latin", W, H, tile, n)["ids"]
        assert ids == [np.nonzero(owner == r)[0].tolist() for r in range(n)]


# ---------------------------------------------------------------- chunk plan

def test_chunk_plan_properties(built):
    cases = []
    for T in (1, 2, 7, 20, 64, 1000):
        for n_slots in (64, 4096, 1 << 22, 1 << 30):
            for per_slot in (28, 44):   # radiance + ray, + per-ray origin
                b = per_slot * n_slots
                for budget in (b // 2, b, 3 * b + 5, (T // 2 + 1) * b, T * b, 10 * T * b):
                    cases.append((T, n_slots, b, budget))
    plans = _run(built, "chunks", *[v for c in cases for v in c])["plans"]
    assert len(plans) == len(cases)
    for (T, n_slots, b, budget), (chunk, launches) in zip(cases, plans):
        sizes = [min(chunk, T - s0) for s0 in range(0, T, chunk)]
        assert sum(sizes) == T and len(sizes) == launches and max(sizes) <= chunk and min(sizes) >= 1
        assert chunk * n_slots < 1 << 31
        assert chunk * b <= budget or chunk == 1
        # the most samples one launch may hold: the budget's (at least one), the 2^31 item bound's
        cap = min(max(1, budget // b), ((1 << 31) - 1) // n_slots, T)
        assert launches == -(-T // cap), (T, n_slots, b, budget, chunk, launches)


def test_chunk_plan_worked_case(built):
    # 4096 slots at 28 B per slot and sample, 1 MiB: the budget holds 9 samples, 20 samples take
    # three launches, evened out to 7, 7, 6
    assert (1 << 20) // (28 * 4096) == 9
    assert _run(built, "chunks", 20, 4096, 28 * 4096, 1 << 20)["plans"] == [[7, 3]]
    assert [l[1] for l in _run(built, "frames", 20, 1, 7)["launches"]] == [7, 7, 6]


@pytest.mark.parametrize("chunk", [7, 20, 100], ids=["straddles_three_frames", "chunk_eq_T", "chunk_gt_T"])
def test_frame_windows_of_a_launch(built, chunk):
    spp, n_frames = 4, 5
    T = spp * n_frames
    got = _run(built, "frames", spp, n_frames, chunk)["launches"]
    want = [[s0, min(chunk, T - s0), s0 // spp, min(n_frames, -(-(s0 + min(chunk, T - s0)) // spp))]
            for s0 in range(0, T, chunk)]
    assert got == want
    if chunk == 7:
        assert got[1] == [7, 7, 1, 4]   # samples 7..13: frames 1, 2 and 3
    else:
        assert got == [[0, T, 0, n_frames]]


# ---------------------------------------------------------------- LDS layouts and the variant choice
# The layouts of prt_lds_layout.h and the size-only launch decisions of prt_plan.cpp against the four
# statements they replaced, restated here from their text: trace_kernel's and trace_kernel_pool's pointer
# chains, lds_scene_bytes() and trace_smem_bytes(), and the rules of lds_fits4 / default_variant /
# launch_variant.  Sizes are (n_node_f4, n_tri_f4, n_tri, n_mat, n_lt, n_light, stack) as int64.

KB = 256                      # kBlock
POOL_F4, QUEUE_F4, CTL_F4 = 7 * KB // 4, 2 * KB // 16, 3
LDS_VARS, POOL_VARS = (1, 2, 4, 6, 7, 8), (7, 8)


def _sizes(n_node4=1, n_refs=1, n_tri=1, n_mat=1, n_lt=1, n_light=1, stack=1):
    """A size tuple from counts: whole BVH4 nodes of 8 float4 (the layouts' precondition n_node_f4 % 8 == 0)
    and triangle records of 3 float4."""
    return np.array([8 * n_node4, 3 * n_refs, n_tri, n_mat, n_lt, n_light, stack], np.int64)


def _old_scene_bytes(z):
    nn, tf4, nt, nm, nlt, nl, _ = z
    return 16 * (7 * nn + tf4 + 7 * nt + 2 * nm + 4 * nlt) + 4 * (nl + 1)


def _old_smem(stack, var, z):
    nn, tf4, nt, nm, nlt, nl, lds_stack = z
    if var in POOL_VARS:
        return (lds_stack * KB * 2 + 16 * (POOL_F4 + QUEUE_F4 + CTL_F4) +
                16 * (7 * nn + tf4 + 4 * nlt + (nl + 4) // 4 + 2 * nm))
    b = stack * KB * (2 if var in LDS_VARS else 4)
    return b + _old_scene_bytes(z) if var in LDS_VARS else b


def _old_trace_regions(z):
    """trace_kernel's pointer chain: (float4 offset, bytes its copy loop fills) per region, in order."""
    nn, tf4, nt, nm, nlt, nl, stack = z
    sn = stack * KB * 2 // 16
    st4 = sn + 56 * (nn // 8)
    snm = st4 + tf4
    sfr = snm + nt
    smt = sfr + 6 * nt
    slv = smt + 2 * nm
    slo = slv + 4 * nlt
    return [(0, stack * KB * 2), (sn, 16 * 56 * (nn // 8)), (st4, 16 * tf4), (snm, 16 * nt), (sfr, 16 * 6 * nt),
            (smt, 16 * 2 * nm), (slv, 16 * 4 * nlt), (slo, 4 * (nl + 1))]


def _old_pool_regions(z):
    """trace_kernel_pool's pointer chain, likewise."""
    nn, tf4, nt, nm, nlt, nl, stack = z
    pool = stack * KB * 2 // 16
    queue = pool + POOL_F4
    ctl = pool + POOL_F4 + QUEUE_F4
    sn = pool + POOL_F4 + QUEUE_F4 + CTL_F4
    st4 = sn + 56 * (nn // 8)
    slv = st4 + tf4
    slo = slv + 4 * nlt
    smt = slv + 4 * nlt + (nl + 4) // 4
    return [(0, stack * KB * 2), (pool, 4 * 7 * KB), (queue, 2 * KB), (ctl, 4 * 12), (sn, 16 * 56 * (nn // 8)),
            (st4, 16 * tf4), (slv, 16 * 4 * nlt), (slo, 4 * (nl + 1)), (smt, 16 * 2 * nm)]


def _old_fits(z):
    return bool(_old_scene_bytes(z) <= 24 * 1024 and z[0] // 8 < 0x7FFF and (z[1] // 3) * 8 <= 32768)


def _old_variant(z, need4, stack4, mis):
    z = z.copy()
    z[6] = need4   # size_params: P.lds_stack = need4
    lds = _old_fits(z) and stack4 != 0
    if mis:
        return 4 if lds else 5
    if not lds:
        return 3
    if need4 <= 32 and _old_smem(16, 7, z) * 7 <= 160 * 1024:
        return 7
    smem = _old_smem(stack4, 1, z)
    return 1 if smem * 7 <= 160 * 1024 else 6 if smem * 6 <= 160 * 1024 else 2


def _with_total(total, fn, make=_sizes, **counts):
    """The size tuple make(**counts) with n_refs, n_mat and n_lt chosen so that fn(sizes) == total."""
    for n_mat in range(1, 8):
        for n_lt in range(1, 5):
            z0 = make(n_refs=0, n_mat=n_mat, n_lt=n_lt, **counts)
            rest = total - fn(z0)
            if rest >= 48 * counts["n_tri"] and rest % 48 == 0:
                z = make(n_refs=int(rest // 48), n_mat=n_mat, n_lt=n_lt, **counts)
                assert fn(z) == total
                return z
    raise AssertionError("no tuple with total %d" % total)


def _size_tuples():
    t = {"ones": _sizes()}
    for nl in (1, 3, 4, 5):
        t["n_light_%d" % nl] = _sizes(n_node4=3, n_refs=9, n_tri=7, n_mat=2, n_lt=nl + 1, n_light=nl, stack=10)
    t["cornell_sized"] = _sizes(n_node4=11, n_refs=36, n_tri=36, n_mat=8, n_lt=2, n_light=1, stack=10)
    # lds_fits' 24 KiB: the last copy that fits and one float4 more (n_light = 3: a 16-byte offsets tail)
    for total in (24576, 24592):
        t["scene_%d" % total] = _with_total(total, _old_scene_bytes, n_node4=10, n_tri=40, n_light=3, stack=10)
    for n4 in (0x7FFE, 0x7FFF):
        t["n_node4_%#x" % n4] = _sizes(n_node4=n4, n_refs=8, n_tri=8, stack=10)
    for refs in (4096, 4097):
        t["n_refs_%d" % refs] = _sizes(n_node4=2, n_refs=refs, n_tri=8, stack=10)
    # default_variant's 160 KiB steps: the largest total (whole float4: n_light = 3) that passes, and
    # the next.  The pooled kernel at seven blocks; then, with few enough normals and frames that the pooled
    # kernel is already out, the phase-aligned one at seven and at six.
    for total in (23392, 23408):
        assert (total * 7 <= 160 * 1024) == (total == 23392)
        t["pool7_%d" % total] = _with_total(total, lambda z: _old_smem(16, 7, z), n_node4=6, n_tri=60, n_light=3,
                                            stack=10)
        t["lds7_%d" % total] = _with_total(total, lambda z: _old_smem(10, 1, z), n_node4=6, n_tri=20, n_light=3,
                                           stack=10)
    for total in (27296, 27312):
        assert (total * 6 <= 160 * 1024) == (total == 27296)
        t["lds6_%d" % total] = _with_total(total, lambda z: _old_smem(10, 1, z), n_node4=6, n_tri=20, n_light=3,
                                           stack=10)
    return t


SIZE_TUPLES = _size_tuples()


def test_size_tuples_sit_on_the_thresholds_they_name():
    t = SIZE_TUPLES
    assert _old_fits(t["scene_24576"]) and not _old_fits(t["scene_24592"])
    assert [_old_variant(t[k], 10, 10, False) for k in ("pool7_23392", "pool7_23408")] == [7, 1]
    assert [_old_variant(t[k], 10, 10, False) for k in ("lds7_23392", "lds7_23408", "lds6_27296", "lds6_27312")] == \
        [1, 6, 6, 2]


def test_lds_layouts_match_the_four_statements_they_replaced(built):
    names = list(SIZE_TUPLES)
    reps = _run(built, "layout", *[int(v) for k in names for v in SIZE_TUPLES[k]])
    assert len(reps) == len(names)
    for name, rep in zip(names, reps):
        z = SIZE_TUPLES[name]
        stack = int(z[6])
        for key, regions, total in (("trace", _old_trace_regions(z), _old_smem(stack, 1, z)),
                                    ("pool", _old_pool_regions(z), _old_smem(16, 7, z))):
            off = rep[key]
            assert off == [int(o) for o, _ in regions], (name, key)
            ends = [16 * int(o) + int(b) for o, b in regions]
            # in order and disjoint: a region starts at or after the end of the one before it
            assert all(16 * off[i + 1] >= ends[i] for i in range(len(off) - 1)), (name, key)
            assert off == sorted(off) and off[0] == 0
            # float4-aligned: the offsets are whole float4 by construction; the region before must not
            # reach into the next one's first float4
            assert all(16 * off[i + 1] - ends[i] < 16 for i in range(len(off) - 1)), (name, key)
            assert ends[-1] == rep[key + "_bytes"] == int(total), (name, key)
        assert rep["scene_bytes"] == int(_old_scene_bytes(z)), name
        assert rep["smem"] == [int(_old_smem(stack, var, z)) for var in range(0, 10)], name


def test_variant_choice_matches_the_parent_rule(built):
    cases = []
    for name, z in SIZE_TUPLES.items():
        need4 = int(z[6])
        stack4 = 10 if need4 <= 10 else 16 if need4 <= 16 else 32
        for n4, s4 in ((need4, stack4), (need4, 0), (32, 32), (33, 32)):
            cases.append((name, z, n4, s4))
    reps = _run(built, "variant", *[int(v) for _, z, n4, s4 in cases for v in list(z[:6]) + [n4, s4]])
    assert len(reps) == len(cases)
    seen = set()
    for (name, z, n4, s4), rep in zip(cases, reps):
        zz = z.copy()
        zz[6] = n4
        assert rep["fits"] == _old_fits(zz), (name, n4, s4)
        assert rep["nee"] == _old_variant(z, n4, s4, False), (name, n4, s4)
        assert rep["mis"] == _old_variant(z, n4, s4, True), (name, n4, s4)
        seen.update((rep["nee"], rep["mis"]))
    assert seen == {1, 2, 3, 4, 5, 6, 7}   # every variant a default can be (8 is only ever forced)


# ---------------------------------------------------------------- the width rule
# prt_plan.cpp lds_width restated from its text.  The restatements above extended by the width: a width
# tuple is a size tuple followed by the width, its n_node_f4 counting 14 float4 per BVH8 node, and a
# width-8 node copy is 8 x n_node_f4 where the BVH4's is 7 x n_node_f4.

def _sizes8(n_node8=1, width=8, **counts):
    z = _sizes(n_node4=0, **counts)
    z[0] = 14 * n_node8
    return np.append(z, width)


def _node_copy_extra(z):
    return 16 * z[0] if z[7] == 8 else 0


def _scene_bytes_w(z):
    return _old_scene_bytes(z[:7]) + _node_copy_extra(z)


def _pool_bytes_w(z, stack):
    zz = z[:7].copy()
    zz[6] = stack
    return _old_smem(16, 7, zz) + _node_copy_extra(z)


def _fits_w(z):
    n_nodes = z[0] // (14 if z[7] == 8 else 8)
    return bool(_scene_bytes_w(z) <= 24 * 1024 and n_nodes < 0x7FFF and (z[1] // 3) * 8 <= 32768)


def _width_rule(z, need8, knob):
    can8 = z[7] == 8 and z[0] > 0 and 1 <= need8 <= 32 and _fits_w(z)
    if not can8 or knob == 4:
        return 4
    if knob == 8:
        return 8
    return 8 if _pool_bytes_w(z, need8) * 7 <= 160 * 1024 else 4


def _width_cases():
    """(what the case names, width tuple, need8, knob, the width it claims)."""
    box = dict(n_node8=3, n_refs=36, n_tri=36, n_mat=8, n_lt=2, n_light=1, stack=15)   # the Cornell box's BVH8
    c = [("need8_%d" % need8, _sizes8(**box), need8, 8, want) for need8, want in ((0, 4), (1, 8), (32, 8), (33, 4))]
    c += [("need8_1_default", _sizes8(**box), 1, 0, 8),
          ("need8_32_default", _sizes8(**box), 32, 0, 4)]      # 16 KiB of stacks: seven blocks no longer fit
    for total, want in ((24576, 8), (24592, 4)):
        z = _with_total(total, _scene_bytes_w, make=_sizes8, n_node8=5, n_tri=40, n_light=3, stack=10)
        c.append(("scene_%d" % total, z, 10, 8, want))
    for total, want in ((23392, 8), (23408, 4)):
        z = _with_total(total, lambda z: _pool_bytes_w(z, 10), make=_sizes8, n_node8=3, n_tri=36, n_light=3, stack=10)
        c += [("pool7_%d" % total, z, 10, 0, want), ("pool7_%d_knob5" % total, z, 10, 5, want),
              ("pool7_%d_forced" % total, z, 10, 8, 8)]
    c += [("z8_width_4_knob%d" % knob, _sizes8(width=4, **box), 15, knob, 4) for knob in (0, 8)]
    c += [("no_bvh8_knob%d" % knob, _sizes8(**dict(box, n_node8=0)), 15, knob, 4) for knob in (0, 8)]
    c += [("knob_%d" % knob, _sizes8(**box), 15, knob, want) for knob, want in ((0, 8), (4, 4), (8, 8), (5, 8))]
    return c


WIDTH_CASES = _width_cases()


def test_width_tuples_sit_on_the_thresholds_they_name():
    by_name = {name: (z, need8, knob, want) for name, z, need8, knob, want in WIDTH_CASES}
    assert len(by_name) == len(WIDTH_CASES)
    for name, (z, need8, knob, want) in by_name.items():
        assert _width_rule(z, need8, knob) == want, name
    for total in (24576, 24592):
        z = by_name["scene_%d" % total][0]
        assert _scene_bytes_w(z) == total and _fits_w(z) == (total == 24576)
        assert _scene_bytes_w(z) - _old_scene_bytes(z[:7]) == 5 * 224     # the eighth copy of five nodes' 14 float4
        assert _pool_bytes_w(z, 10) * 7 > 160 * 1024                      # so only the forced width gets this far
    for total in (23392, 23408):
        z = by_name["pool7_%d" % total][0]
        assert _pool_bytes_w(z, 10) == total and total % 16 == 0 and _fits_w(z)
        assert (total * 7 <= 160 * 1024) == (total == 23392)
    box = by_name["knob_0"][0]
    assert _fits_w(box) and _pool_bytes_w(box, 15) * 7 <= 160 * 1024 < _pool_bytes_w(box, 32) * 7
    assert by_name["z8_width_4_knob8"][0][7] == 4 and by_name["no_bvh8_knob8"][0][0] == 0
    assert {want for *_, want in WIDTH_CASES} == {4, 8}


def _widths(built, cases):
    """lds_width of (width tuple, need8, knob) triples through the stand-alone driver."""
    got = _run(built, "width", *[int(v) for z, need8, knob in cases for v in list(z) + [need8, knob]])["width"]
    assert len(got) == len(cases)
    return got


def test_width_rule_matches_its_restatement(built):
    got = _widths(built, [(z, need8, knob) for _, z, need8, knob, _ in WIDTH_CASES])
    for (name, z, need8, knob, want), w in zip(WIDTH_CASES, got):
        assert w == want == _width_rule(z, need8, knob), (name, w, want)


def test_width_rule_on_the_real_scenes(built, cornell):
    """The sizes of the Cornell box and of the two hostile LDS-resident scenes, from the builder's own
    collapse: the default rule picks 8 for the box and 4 for the others, whose eight-wide pooled layout no
    longer fits seven blocks per CU; forced, all three run at width 8 (tests/test_gpu_lds_width_hard.py)."""
    import hard_scenes as HS
    from pyrenderer_amd import _native as N
    cases = []
    for name in ("cornell", "layers-0", "slivers8-1e-5"):
        flat = HS.case(cornell, name)[0]
        b = N.Bvh(flat.tri_v, max_leaf=4)
        nodes8, _, need8 = b.collapse(8)
        z8 = np.array([14 * len(nodes8), 3 * b.n_tri, flat.n_tri, flat.mat.shape[0], flat.light_tri.shape[0],
                       flat.n_light, need8, 8], np.int64)
        assert _fits_w(z8) and need8 <= 32, name
        print(name, "BVH8 nodes", len(nodes8), "need", need8, "scene bytes", _scene_bytes_w(z8), "pooled",
              _pool_bytes_w(z8, need8))
        cases += [(z8, need8, knob) for knob in (0, 4, 8)]
    got = _widths(built, cases)
    assert got == [_width_rule(*c) for c in cases]
    assert got == [8, 4, 8, 4, 4, 8, 4, 4, 8], got


# ---------------------------------------------------------------- knobs and camera

def test_env_int_clamps_and_falls_back(built):
    assert _run(built, "env", "PRT_T_UNSET", 0, 64, -1)["value"] == -1
    assert _run(built, "env", "PRT_T", 0, 64, -1, PRT_T="100")["value"] == 64
    assert _run(built, "env", "PRT_T", 1, 64, 32, PRT_T="-5")["value"] == 1
    assert _run(built, "env", "PRT_T", 0, 64, 12, PRT_T="abc")["value"] == 0
    assert _run(built, "env", "PRT_T", 1, 0xFFFFFFFF, 1 << 20, PRT_T="99999999999")["value"] == 0xFFFFFFFF
    assert _run(built, "env", "PRT_T", 1 << 20, (1 << 63) - 1, 0, PRT_T=str(1 << 34))["value"] == 1 << 34
    assert _run(built, "env", "PRT_T", 1 << 20, (1 << 63) - 1, 0, PRT_T="4096")["value"] == 1 << 20
    spill = [_run(built, "env", "PRT_T", -(1 << 31), (1 << 31) - 1, 16, PRT_T=v)["spill_lds"] for v in "4 16 32 7 0".split()]
    assert spill == [4, 16, 32, 16, 16]
    assert _run(built, "env", "PRT_T_UNSET", -(1 << 31), (1 << 31) - 1, 16)["spill_lds"] == 16


def test_camera_terms_in_f32_order(built, cornell, tmp_path):
    cam = np.ascontiguousarray(cornell[1].convert_to_taichi_camera().packed(), F).copy()

    def check(c):
        p = tmp_path / "cam.f32"
        c.astype(F).tofile(p)
        rep = _run(built, "camera", p)
        fast = bool(np.isfinite(c[:20]).all() and not c[19] > 0 and tuple(c[12:16]) == (0, 0, 0, 1))
        assert rep["fast"] == fast
        with np.errstate(invalid="ignore"):
            rows = c[:12].reshape(3, 4)
            o = ((F(0) * rows[:, 0] + F(0) * rows[:, 1]) + F(0) * rows[:, 2]) + F(1) * rows[:, 3]
            k = -c[18] * rows[:, 2]
        assert rep["cam_o"] == o.astype(F).view(np.uint32).tolist()
        assert rep["cam_k"] == k.astype(F).view(np.uint32).tolist()
        return fast

    pin = cam.copy()
    pin[12:16], pin[19] = (0, 0, 0, 1), 0
    assert check(cam) in (True, False) and check(pin)
    for i, v in ((19, 0.5), (12, 0.25), (3, np.inf)):   # thin lens, projective row, non-finite
        c = pin.copy()
        c[i] = v
        assert not check(c)


# ---------------------------------------------------------------- scene validation and packing

def _packed(d, name, width):
    return np.fromfile(os.path.join(d, name + ".f32"), F).reshape(-1, width)


@pytest.mark.parametrize("name,args,message", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_scene_reports_its_first_failed_check(built, tmp_path, name, args, message):
    assert _scene(built, str(tmp_path), args) == {"error": message}


def _norm(n):
    """f3_norm in numpy f32, in its operation order."""
    n = n.astype(F)
    l = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return np.array([n[0] / l, n[1] / l, n[2] / l], F)


def _check_packing(d, s, rep):
    n_tri = s["n_tri"]
    tri_n, tri_v, tri_mat = s["tri_n"].reshape(-1, 3), s["tri_v"].reshape(-1, 9), s["tri_mat"]
    nm = _packed(d, "tri_nm", 4)
    assert nm.shape[0] == n_tri
    assert np.array_equal(nm[:, :3].view(np.uint32), tri_n.view(np.uint32))
    assert np.array_equal(nm[:, 3].view(np.int32), tri_mat)
    fr = _packed(d, "tri_frame", 12).reshape(n_tri, 2, 3, 4)
    assert not fr[..., 3].any()
    for i in range(n_tri):
        for side, n in enumerate((tri_n[i], -tri_n[i])):
            rows = fr[i, side, :, :3]
            v = _norm(n)
            if v[1] in (1, -1):
                assert np.array_equal(rows, np.array([[1, 0, 0], [0, 0, 1], [0, v[1], 0]], F))
            else:
                assert np.array_equal(rows[2].view(np.uint32), v.view(np.uint32))   # rows x, z, v
                assert np.abs(rows.astype(np.float64) @ rows.astype(np.float64).T - np.eye(3)).max() <= 1e-6
                assert rows[0, 1] == 0   # x = normalize(v x (0,1,0)) lies in the xz plane
    n_lt = int(s["light_off"][s["n_light"]])
    assert rep["n_lt"] == n_lt
    lv = _packed(d, "light_v", 16)
    assert lv.shape[0] == n_lt
    t = s["light_tri"][:n_lt]
    for k in range(3):
        assert np.array_equal(lv[:, 4 * k:4 * k + 3], tri_v[t, 3 * k:3 * k + 3]) and not lv[:, 4 * k + 3].any()
    assert np.array_equal(lv[:, 12:15], tri_n[t]) and np.array_equal(lv[:, 15].view(np.int32), tri_mat[t])


def test_cornell_packs_as_the_kernels_read_it(built, cornell, tmp_path):
    s = _flat_args(cornell[2])
    rep = _scene(built, str(tmp_path), s)
    assert rep["error"] is None and rep["plain"] is True and rep["shade_fast"] is True
    _check_packing(str(tmp_path), s, rep)


def _hand_made(**over):
    """Three triangles: normals +y, -y and a non-unit one; the second emits."""
    tri_v = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 1], [0, 2, 0, 0, 2, 1, 1, 2, 0], [0, 0, 0, 0, 1, 0, 1, 0, 0]], F)
    s = scene(tri_v=tri_v, tri_n=np.array([[0, 1, 0], [0, -1, 0], [0.6, 1.2, -0.5]], F), tri_mat=np.array([0, 1, 0], np.int32),
              n_tri=3, mat=np.array([[0.5, 0.25, 0.75, 0, 0, 0, 1, 0], [1, 1, 1, 5, 0, 0, 1, 0]], F), n_mat=2,
              light_tri=np.array([1], np.int32), light_off=np.array([0, 1], np.int32), n_light=1)
    s.update(over)
    return s


def test_hand_made_scene_packs_the_literal_y_frames(built, tmp_path):
    s = _hand_made()
    rep = _scene(built, str(tmp_path), s)
    assert rep["error"] is None and rep["plain"] is True and rep["shade_fast"] is True
    _check_packing(str(tmp_path), s, rep)
    fr = _packed(str(tmp_path), "tri_frame", 12).reshape(3, 2, 3, 4)
    up = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0]], F)
    down = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], F)
    assert np.array_equal(fr[0], [up, down]) and np.array_equal(fr[1], [down, up])


def _mat(s, row, col, value):
    m = s["mat"].copy()
    m[row, col] = value
    return m


@pytest.mark.parametrize("over,plain,shade_fast", [
    (lambda s: dict(mat=_mat(s, 0, 5, 2)), False, True),                                      # metal
    (lambda s: dict(mat=_mat(s, 1, 5, 3)), False, True),                                      # dielectric
    (lambda s: dict(sph=np.array([[0, 0, 0, 1]], F), sph_mat=np.array([0], np.int32), n_sph=1), False, True),
    (lambda s: dict(mat=_mat(s, 0, 1, 0)), True, False),                                      # albedo 0
    (lambda s: dict(mat=_mat(s, 0, 2, 1e-20)), True, False),                                  # albedo 1e-20
    (lambda s: dict(tri_n=np.array([[0, 1, 0], [0, -1, 0], [1, 2, 2]], F)), True, False),     # normal of length 3
], ids=["metal", "dielectric", "sphere", "albedo_0", "albedo_1e-20", "normal_length_3"])
def test_plain_and_shade_fast_classification(built, tmp_path, over, plain, shade_fast):
    s = _hand_made()
    s.update(over(s))
    rep = _scene(built, str(tmp_path), s)
    assert rep["error"] is None and (rep["plain"], rep["shade_fast"]) == (plain, shade_fast)


def test_valid_base_scene_is_accepted(built, tmp_path):
    rep = _scene(built, str(tmp_path), base_scene())
    assert rep == {"error": None, "n_lt": 1, "plain": True, "shade_fast": True}

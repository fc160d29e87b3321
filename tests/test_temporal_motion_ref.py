"""The NumPy restatement of the temporal accumulation (tests/temporal_ref.py) with ids and per-object motion
against what can be known without them: the same function without ids wherever no pixel has a row, bit for bit
(tests/test_temporal_ref.py anchors that form), and float64 geometry on the analytic card scene
(tests/temporal_motion_cases.py).

The restatement's figures on the clean card scene at 70 x 130: card pixels that accept history with the card's
row 0.9762 (static) and 0.7623 (moved), with an identity row in its place 0.0000 and 0.0000; greatest error of
px, py against float64 2.5e-5 pixel."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_motion_cases as MC
import temporal_ref as T
from denoise_cases import MARKER, bits

F32 = np.float32
SHAPES = [(1, 1), (3, 7), (33, 17), (70, 130)]
P = T.DEFAULTS


def _same(got, want):
    for g, w in zip(got[:3], want[:3]):
        diff = np.argwhere(bits(g) != bits(w))
        assert len(diff) == 0, (len(diff), diff[:5])


@pytest.fixture(scope="module")
def plain():
    """temporal_cases.hostile and the restatement's result without ids for every shape and kind, computed once."""
    out = {}
    for W, H in SHAPES:
        for kind in TC.KINDS:
            C, F, cam, prev = TC.hostile(kind, W, H)
            out[(W, H, kind)] = (C, F, cam, prev, T.accumulate(C, F, cam, prev, **P))
    return out


def _with_ids(prev, pids):
    return None if prev is None else (*prev, pids)


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_without_a_row_it_is_the_static_restatement(plain, W, H, kind):
    """One id on both frames that has no row, or the identity's, is no id plane at all."""
    C, F, cam, prev, want = plain[(W, H, kind)]
    none = np.full((W, H), -1, np.int32)
    # an empty table and every id -1
    _same(T.accumulate(C, F, cam, _with_ids(prev, none), ids=none, motion=None, **P), want)
    # every id out of range, each kind of it, against a table that holds rows nobody may read
    table = MC.motion_table()
    for v in MC.BAD_IDS:
        out = np.full((W, H), v, np.int32)
        _same(T.accumulate(C, F, cam, _with_ids(prev, out), ids=out, motion=table, **P), want)
    # every id 0 and one bytewise identity row
    zero = np.zeros((W, H), np.int32)
    _same(T.accumulate(C, F, cam, _with_ids(prev, zero), ids=zero, motion=T.IDENTITY[None], **P), want)


@pytest.fixture(scope="module")
def cards():
    out = {}
    for kind in ("static", "moved"):
        C, F, cam, ids, motion, prev = MC.clean(kind, 70, 130)
        out[kind] = (C, F, cam, ids, motion, prev, T.accumulate(C, F, cam, prev, ids=ids, motion=motion, diagnostics=True, **P))
    return out


@pytest.mark.parametrize("kind", ("static", "moved"))
def test_the_card_keeps_its_history_only_with_its_row(cards, kind):
    C, F, cam, ids, motion, prev, (state, _, _, d) = cards[kind]
    card = ids == MC.CARD
    assert card.sum() > 1000
    share = float(d["valid"][card].mean())
    still = motion.copy()
    still[MC.CARD] = T.IDENTITY
    s2 = T.accumulate(C, F, cam, prev, ids=ids, motion=still, **P)[0]
    share_still = float((s2[..., 3][card] > 1).mean())
    # float64 reprojection of the card's pixels through its matrix
    px, py = MC.project64(F, cam, prev[2], MC.card_motion())
    err = max(float(np.abs(d["px"][card] - px[card]).max()), float(np.abs(d["py"][card] - py[card]).max()))
    print(f"card scene {kind}: share with the card's row {share:.4f}, with an identity row {share_still:.4f}, "
          f"greatest px / py error {err:.2e}")
    assert share >= 0.7 and (state[..., 3][card & d["valid"]] > 1).all()
    assert share_still <= 0.05
    assert err <= 1e-3
    assert not d["one_tap"][card].any()


def test_rows_that_are_not_finite_reset_and_the_minus_zero_row_goes_the_long_way(cards):
    for kind in ("static", "moved"):
        C, F, cam, ids, motion, prev, (state, _, var, d) = cards[kind]
        for oid in (MC.CARD_NAN, MC.CARD_INF):
            m = ids == oid
            assert m.sum() > 20 and d["no_pose"][m].all()
            assert (state[m, 3] == 1).all() and (bits(var[m]) == MARKER).all() and not d["valid"][m].any()
        m = ids == MC.CARD_NEG0
        assert m.sum() > 20 and not d["one_tap"][m].any() and not d["no_pose"][m].any()
    # equal cameras: the card stands still in the image with the -0 row, and the long way finds its history
    C, F, cam, ids, motion, prev, (state, _, _, d) = cards["static"]
    m = ids == MC.CARD_NEG0
    inner = m & np.roll(m, 1, 0) & np.roll(m, -1, 0) & np.roll(m, 1, 1) & np.roll(m, -1, 1)
    assert inner.sum() > 10 and d["valid"][inner].all()
    assert d["one_tap"][ids == MC.GROUND].all()


def test_under_equal_cameras_ground_uncovered_by_the_card_starts_afresh(cards):
    C, F, cam, ids, motion, prev, (state, _, _, d) = cards["static"]
    uncovered = (ids == MC.GROUND) & (prev[3] == MC.CARD)
    kept = (ids == MC.GROUND) & (prev[3] == MC.GROUND)
    assert uncovered.sum() > 100 and (state[uncovered, 3] == 1).all()
    # ... and the ground that stayed ground is the exact one-tap running update
    assert kept.sum() > 1000 and np.array_equal(state[kept, 3], prev[0][kept, 3] + 1)


@pytest.mark.parametrize("kind", TC.KINDS)
def test_the_hostile_scene_exercises_every_branch(kind):
    W, H = 70, 130
    C, F, cam, ids, motion, prev = MC.hostile(kind, W, H)
    state, color, var, d = T.accumulate(C, F, cam, prev, ids=ids, motion=motion, diagnostics=True, **P)
    for v in MC.BAD_IDS:
        assert (ids == v).sum() > 50, v
    for oid in range(MC.N_OBJECTS):
        assert (ids == oid).sum() > 20, oid
    bad = T.prepare(C, F, P["eps_a"])[6]
    assert bad.any() and not state[bad].any()
    if prev is None:
        assert (state[~bad, 3] == 1).all()
        return
    invalid = np.isin(ids, MC.BAD_IDS)
    if kind == "static":
        assert (d["valid"] & invalid).any()          # an id without a row accepts when the previous id agrees
        assert (d["valid"] & (ids == MC.CARD)).any() and (d["valid"] & (ids == MC.GROUND)).any()
        assert (~d["valid"] & d["one_tap"] & (ids != prev[3])).any()
    if kind == "moved":
        assert (d["valid"] & (ids == MC.CARD)).any() and (d["valid"] & (ids == MC.GROUND)).any()
    if kind == "behind":
        assert d["valid"].mean() < 0.05
    assert not d["valid"][d["no_pose"]].any()


def test_the_librarys_rows_are_the_restatements():
    """What pyrenderer_amd.denoise.motion_rows writes for a primitive that stands still is the row the restatement
    (and the kernel) take the one-tap shortcut for, and a primitive without a rigid motion gets "no previous pose"."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd import scenes as S
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    assert D.IDENTITY_ROW.tobytes() == T.IDENTITY.tobytes()
    scene = read_file(S.CORNELL)[0]
    later = S.moved(scene, {5: S.spin(scene.primitives[5], 6.0)})
    rows = D.motion_rows(scene, later)
    rows[6] = np.nan
    ids = np.arange(8, dtype=np.int32).reshape(2, 4)
    _, has_row, no_pose, identity = T.rows_of(ids, rows)
    assert has_row.all() and np.array_equal(no_pose.reshape(-1), np.arange(8) == 6)
    assert np.array_equal(identity.reshape(-1), ~np.isin(np.arange(8), (5, 6)))

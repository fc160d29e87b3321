"""The adaptive-sampling restatement (tests/adaptive_ref.py) and the stop policy
(pyrenderer_amd.adaptive.still_active) without a GPU: the restatement against moments_ref, the tiles it
leaves alone, the records' independence of the list's order, and the policy's edges."""
import numpy as np
import pytest

import adaptive_ref as A
import moments_ref as M
from denoise_cases import bits

F32 = np.float32
SENTINEL = np.uint32(0x7FC12345)   # a NaN with a payload: any arithmetic on it would change the bits


def _inputs(W, H, seed):
    rng = np.random.default_rng(seed)
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = rng.uniform(0.02, 1.0, (W, H, 3))
    F[..., 7] = rng.choice([0.0, 0.5, 1.0], (W, H))
    frames = (4.0 * rng.uniform(0.1, 1.5, (3, W, H, 3))).astype(F32)
    return F, frames


def _run(W, H, tw, th, ids, frames, F, target=0.05, fill=None):
    """Three batches of the tiles `ids` through update(); `fill`: the bits every plane starts with."""
    s = np.zeros((W, H, 3), F32)
    st = np.zeros((W, H, 4), F32)
    if fill is not None:
        s.view(np.uint32)[...] = fill
        st.view(np.uint32)[...] = fill
        for tid in ids:   # the listed tiles start empty
            x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
            s[x0:x0 + w, y0:y0 + h] = 0
            st[x0:x0 + w, y0:y0 + h] = 0
    recs = []
    for fr in frames:
        s, st, r = A.update(s, st, A.pack(fr, ids, tw, th), ids, tw, th, F, 4.0, 1e-2, 1e-3, target)
        recs.append(r)
    return s, st, recs


@pytest.mark.parametrize("W,H,tw,th", [(13, 9, 8, 8), (37, 19, 16, 4), (70, 40, 64, 64)])
def test_full_list_equals_moments_ref_bit_for_bit(W, H, tw, th):
    F, frames = _inputs(W, H, 7 + W)
    ids = np.arange(A.n_tiles(tw, th, W, H))
    s, st, recs = _run(W, H, tw, th, ids, frames, F)
    want = M.moments_add(np.zeros((W, H, 4), F32), frames, 4.0, F, 1e-2)
    assert np.array_equal(bits(st), bits(want))
    assert np.array_equal(bits(s), bits((frames[0] + frames[1]) + frames[2]))
    # pack and unpack are inverse on the frame, and the records count what they say
    assert np.array_equal(A.unpack(A.pack(frames[0], ids, tw, th), ids, tw, th, W, H), frames[0])
    assert int(recs[0][:, 0].sum()) == W * H
    assert np.array_equal(recs[0][:, 3], recs[0][:, 0]) and np.array_equal(recs[0][:, 1], recs[0][:, 0])   # all young
    assert not recs[0][:, 2].any() and not recs[1][:, 3].any() and recs[1][:, 2].all()
    e = A.relative_error(st, 1e-3)
    for j, tid in enumerate(ids):
        x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
        r = e[x0:x0 + w, y0:y0 + h]
        assert recs[2][j, 2] == r.max().view(np.uint32) and recs[2][j, 1] == (r > F32(0.05)).sum()


def test_unlisted_tiles_keep_a_sentinel():
    W, H, tw, th = 37, 19, 16, 4
    F, frames = _inputs(W, H, 11)
    ids = np.array([7, 0, 12, 3])
    s, st, _ = _run(W, H, tw, th, ids, frames, F, fill=SENTINEL)
    listed = np.zeros((W, H), bool)
    for tid in ids:
        x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
        listed[x0:x0 + w, y0:y0 + h] = True
    assert (bits(s)[~listed] == SENTINEL).all() and (bits(st)[~listed] == SENTINEL).all()
    full = _run(W, H, tw, th, np.arange(A.n_tiles(tw, th, W, H)), frames, F)
    assert np.array_equal(bits(s)[listed], bits(full[0])[listed])
    assert np.array_equal(bits(st)[listed], bits(full[1])[listed])


def test_records_do_not_depend_on_the_order_of_the_list():
    W, H, tw, th = 37, 19, 16, 4
    F, frames = _inputs(W, H, 13)
    ids = np.arange(A.n_tiles(tw, th, W, H))
    perm = np.random.default_rng(5).permutation(len(ids))
    a = _run(W, H, tw, th, ids, frames, F)
    b = _run(W, H, tw, th, ids[perm], frames, F)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    for ra, rb in zip(a[2], b[2]):
        assert np.array_equal(ra[perm], rb)


# ------------------------------------------------------------------ the policy ----

def _rec(n, over, e, young=0):
    return np.array([[n, over, np.float32(e).view(np.uint32), young]], np.uint32)


def test_policy_edges():
    from pyrenderer_amd.adaptive import still_active
    W, H, tw, th = 13, 9, 8, 8
    F, frames = _inputs(W, H, 17)
    ids = np.arange(A.n_tiles(tw, th, W, H))
    # target 0 never stops a tile whose e > 0; +inf stops every tile at min_batches
    zero = _run(W, H, tw, th, ids, frames, F, target=0.0)[2]
    inf = _run(W, H, tw, th, ids, frames, F, target=np.inf)[2]
    for b in (1, 2, 3):
        e = zero[b - 1][:, 2].view(np.float32)
        assert (b == 1 or (e > 0).all()) and still_active(zero[b - 1], b, 2, 0.0).all()
        assert np.array_equal(still_active(inf[b - 1], b, 2, 0.0), np.full(len(ids), b < 2))
        assert still_active(inf[b - 1], b, 3, 0.0).all() == (b < 3)
    assert not inf[1][:, 1].any() and np.array_equal(inf[0][:, 1], inf[0][:, 0])
    # young pixels hold a tile whatever the target: they count as over
    assert still_active(_rec(64, 1, 0.0, young=1), 5, 2, 0.0).all()
    assert not still_active(_rec(64, 0, 0.0), 5, 2, 0.0).any()
    # tolerate rounds down: floor(0.1 * 64) = 6, floor(0.1 * 9) = 0
    assert not still_active(_rec(64, 6, 1.0), 2, 2, 0.1).any() and still_active(_rec(64, 7, 1.0), 2, 2, 0.1).all()
    assert still_active(_rec(9, 1, 1.0), 2, 2, 0.1).all() and not still_active(_rec(9, 0, 1.0), 2, 2, 0.1).any()
    assert not still_active(_rec(64, 63, 1.0), 2, 2, 0.99).any()   # floor(63.36) = 63
    assert still_active(np.zeros((0, 4), np.uint32), 2).shape == (0,)


@pytest.mark.parametrize("kw,word", [
    (dict(min_batches=1), "min_batches"), (dict(min_batches=0), "min_batches"), (dict(min_batches=2.0), "min_batches"),
    (dict(min_batches=True), "min_batches"), (dict(tolerate=1.0), "tolerate"), (dict(tolerate=-0.1), "tolerate"),
    (dict(tolerate=np.nan), "tolerate")])
def test_policy_rejects_bad_parameters(kw, word):
    from pyrenderer_amd.adaptive import still_active
    with pytest.raises(ValueError, match=word):
        still_active(np.zeros((1, 4), np.uint32), 2, **kw)
    with pytest.raises(ValueError, match="records"):
        still_active(np.zeros((4,), np.uint32), 2)


def test_a_stopped_tile_stays_stopped():
    """The sampler's bookkeeping with the device step replaced by the restatement: a tile whose record passes
    once is never listed again, even if a later batch would have put it over the target."""
    from pyrenderer_amd.adaptive import still_active
    W, H, tw, th = 37, 19, 16, 4
    F, frames = _inputs(W, H, 19)
    n = A.n_tiles(tw, th, W, H)
    full = _run(W, H, tw, th, np.arange(n), frames, F, target=0.0)[2]
    target = np.sort(full[1][:, 2])[n // 2].view(np.float32)   # the median tile's worst pixel after two batches
    active, per_tile = np.ones(n, bool), np.zeros(n, np.int32)
    s, st = np.zeros((W, H, 3), F32), np.zeros((W, H, 4), F32)
    listed = []
    for b, fr in enumerate(frames, 1):
        ids = np.nonzero(active)[0]
        listed.append(ids)
        s, st, rec = A.update(s, st, A.pack(fr, ids, tw, th), ids, tw, th, F, 4.0, 1e-2, 1e-3, target)
        per_tile[ids] = b
        active[ids] = still_active(rec, b, 2, 0.0)
    assert set(per_tile.tolist()) == {2, 3} and len(listed[2]) < len(listed[1]) == n
    assert set(listed[2]) <= set(listed[1])
    k = st[..., 0]
    for tid in range(n):
        x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
        assert (k[x0:x0 + w, y0:y0 + h] == per_tile[tid]).all()

"""NumPy float32 restatement of the adaptive-sampling kernel (pyrenderer_amd/csrc/prt_denoise.hip:
adaptive_kernel), a helper module like moments_ref.py.

`update(io_sum, io_state, batch, tile_ids, tw, th, feat, n_samples, eps_a, eps_r, target)` returns what
prt_adaptive_update leaves in io_sum and io_state and writes into records, bit for bit, as new arrays.

per pixel of every listed tile that lies inside the frame, S the pixel's slot of the batch
    io_sum_c = io_sum_c + S_c
    state    = moments_ref.moments_add(state, S, n_samples, feat, eps_a)       (one frame, closing step included)
    e        = sqrt(var_mean if var_mean > 0 else 0) / (|mean| + eps_r)
    young    = k < 2;  over = young or e > target
per listed tile
    records  = (pixels inside the frame, pixels over, max of the bits of e over the pixels that are not young
                or 0, young pixels)

`unpack` / `pack` move between the slot order of the render calls (tile-major, then row ly, then column lx)
and frames [x][y]; `tile_rect` is a tile's part of the frame.
"""
import numpy as np

import moments_ref as M

F32 = np.float32


def tile_rect(tid, tw, th, W, H):
    """(x0, y0, w, h) of tile `tid` clipped to the W x H frame."""
    tiles_x = (W + tw - 1) // tw
    x0, y0 = (int(tid) % tiles_x) * tw, (int(tid) // tiles_x) * th
    return x0, y0, min(tw, W - x0), min(th, H - y0)


def n_tiles(tw, th, W, H):
    return ((W + tw - 1) // tw) * ((H + th - 1) // th)


def pack(frame, tile_ids, tw, th):
    """The slots (n_tiles * tw * th, C) of the tiles `tile_ids` of a frame (W, H, C); slots outside it hold 0."""
    W, H, C = frame.shape
    out = np.zeros((len(tile_ids), th, tw, C), frame.dtype)
    for j, tid in enumerate(tile_ids):
        x0, y0, w, h = tile_rect(tid, tw, th, W, H)
        out[j, :h, :w] = frame[x0:x0 + w, y0:y0 + h].transpose(1, 0, 2)
    return out.reshape(-1, C)


def unpack(slots, tile_ids, tw, th, W, H):
    """The frame (W, H, C) of the slots of the tiles `tile_ids`; zeros elsewhere."""
    C = slots.shape[-1]
    s = np.asarray(slots).reshape(len(tile_ids), th, tw, C)
    frame = np.zeros((W, H, C), s.dtype)
    for j, tid in enumerate(tile_ids):
        x0, y0, w, h = tile_rect(tid, tw, th, W, H)
        frame[x0:x0 + w, y0:y0 + h] = s[j, :h, :w].transpose(1, 0, 2)
    return frame


def relative_error(state, eps_r):
    """e of every pixel of a moments state, (W, H) float32."""
    vm, mean = state[..., 3], state[..., 1]
    with np.errstate(all="ignore"):
        return (np.sqrt(np.where(vm > 0, vm, F32(0.0)).astype(F32)) / (np.abs(mean) + F32(eps_r))).astype(F32)


def update(io_sum, io_state, batch, tile_ids, tw, th, feat, n_samples, eps_a=1e-2, eps_r=1e-3, target=0.05):
    """(sum, state, records): new arrays; records (n_tiles, 4) uint32 in the order of tile_ids."""
    W, H = io_sum.shape[:2]
    tile_ids = np.asarray(tile_ids, np.int64)
    assert len(set(tile_ids.tolist())) == len(tile_ids), "a tile id listed twice"
    S = unpack(np.ascontiguousarray(batch, F32).reshape(-1, 3), tile_ids, tw, th, W, H)
    listed = np.zeros((W, H), bool)
    for tid in tile_ids:
        x0, y0, w, h = tile_rect(tid, tw, th, W, H)
        listed[x0:x0 + w, y0:y0 + h] = True
    with np.errstate(all="ignore"):
        new_sum = np.where(listed[..., None], io_sum + S, io_sum).astype(F32)
    # a NaN of the sentinel survives np.where bit for bit; the state likewise
    new_state = np.where(listed[..., None], M.moments_add(io_state, S, n_samples, feat, eps_a), io_state).astype(F32)
    e = relative_error(new_state, eps_r)
    young = new_state[..., 0] < 2
    with np.errstate(all="ignore"):
        over = young | (e > F32(target))
    e_bits = np.where(young, np.uint32(0), e.view(np.uint32))
    records = np.zeros((len(tile_ids), 4), np.uint32)
    for j, tid in enumerate(tile_ids):
        x0, y0, w, h = tile_rect(tid, tw, th, W, H)
        r = (slice(x0, x0 + w), slice(y0, y0 + h))
        records[j] = (w * h, over[r].sum(), e_bits[r].max(), young[r].sum())
    return new_sum, new_state, records

"""NumPy restatement of the device build of a resident scene's trees (pyrenderer_amd/csrc/prt_lbvh.hip; DESIGN.md
§14), stages 1 to 4 for both widths, word for word; stage 5 (boxes, quantiser) is tests/refit_ref.py's.

The rule (include/prt.h prt_scene_rebuild): centroid c = (lo + hi) * 0.5f of a triangle's vertex bounds; per axis
the cell min(int((c - cmin) / (cmax - cmin) * 1024.0f), 1023) in f32, 0 where the centroids have no extent; the
30-bit Morton code, x the most significant bit of each triple; a stable sort by code is the slot order; the keys
code << 32 | slot are distinct, and a range [a, b] of them splits after the last key that shares with key a every
bit above the highest one in which keys a and b differ (Karras 2012's split, found here by bisection instead of
his per-node search).  A wide node over [a, b] takes the ranges reached after log2(width) such splits, a range
of at most max_leaf slots stopping as a leaf; nodes are numbered breadth-first."""
import numpy as np

import refit_ref as R

F = np.float32
EMPTY = R.EMPTY


def _spread(v):
    v = v.astype(np.uint64) & np.uint64(0x3FF)
    for shift, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def morton_codes(tri_v):
    """(codes (n,) uint32, centroids (n, 3) f32) of the triangles tri_v (n, 9)."""
    v = np.asarray(tri_v, F).reshape(-1, 3, 3)
    if v.shape[0] == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 3), F)
    c = ((v.min(1) + v.max(1)).astype(F) * F(0.5)).astype(F)
    cmin, cmax = c.min(0), c.max(0)
    ext = (cmax - cmin).astype(F)
    u = ((c - cmin).astype(F) / np.where(ext > 0, ext, F(1))).astype(F)
    g = np.minimum((u * F(1024.0)).astype(F).astype(np.int64), 1023)
    g = np.where(ext > 0, g, 0)
    code = (_spread(g[:, 0]) << np.uint64(2)) | (_spread(g[:, 1]) << np.uint64(1)) | _spread(g[:, 2])
    return code.astype(np.uint32), c


def sorted_keys(codes):
    """(order (n,) int32: slot -> triangle, keys: Python ints code << 32 | slot)."""
    order = np.argsort(codes, kind="stable").astype(np.int32)
    keys = [(int(c) << 32) | s for s, c in enumerate(codes[order])]
    return order, keys


def split_of(keys, a, b):
    """The last slot of [a, b]'s left half."""
    bit = (keys[a] ^ keys[b]).bit_length() - 1
    prefix = keys[a] >> bit
    lo, hi = a, b
    while lo < hi:
        m = (lo + hi + 1) // 2
        if keys[m] >> bit == prefix:
            lo = m
        else:
            hi = m - 1
    return lo


def children_of(keys, a, b, max_leaf, width):
    """The slot ranges of the wide node over [a, b], in slot order ([] for the empty range b < a)."""
    if b < a:
        return []
    ch = [(a, b)]
    for _ in range({4: 2, 8: 3}[width]):
        nxt = []
        for x, y in ch:
            if y - x + 1 <= max_leaf:
                nxt.append((x, y))
            else:
                s = split_of(keys, x, y)
                nxt += [(x, s), (s + 1, y)]
        ch = nxt
    return ch


def leaf_ref(first, count):
    return -((first << 3 | (count - 1)) + 1)


def wide_tree(keys, max_leaf, width):
    """dict(nodes (n_nodes, 32 | 56) f32 with the refs set and every box inverted, off (levels + 1,) the level
    offsets, need, depth) of the tree of `width` over the keys."""
    stride = 32 if width == 4 else 56
    level, rows, off, max_anc = [(0, len(keys) - 1, 0)], [], [0], 0
    while level:
        first_below, below = off[-1] + len(level), []
        for a, b, anc in level:
            ch = children_of(keys, a, b, max_leaf, width)
            row = np.zeros(stride, F)
            refs = np.full(width, EMPTY, np.int32)
            for k in range(width):
                for ax in range(3):
                    row[R.plane(k, 2 * ax)], row[R.plane(k, 2 * ax + 1)] = np.inf, -np.inf
            for k, (x, y) in enumerate(ch):
                if y - x + 1 > max_leaf:
                    refs[k] = first_below + len(below)
                    below.append((x, y, anc + len(ch) - 1))
                else:
                    refs[k] = leaf_ref(x, y - x + 1)
            row[6 * width:7 * width] = refs.view(F)
            rows.append(row)
            max_anc = max(max_anc, anc)
        off.append(first_below)
        level = below
    return dict(nodes=np.array(rows, F), off=np.array(off, np.int64), need=1 + max_anc + width - 1, depth=len(off) - 2)


def rebuild(tri_v, max_leaf=4, widths=(4, 8)):
    """Everything the device writes: dict(pad, order, tris, nodes4, nodes4q, nodes8 (None without width 8), off4,
    off8, need4, need8, depth4, depth8)."""
    tri_v = np.asarray(tri_v, F).reshape(-1, 9)
    codes, _ = morton_codes(tri_v)
    order, keys = sorted_keys(codes)
    pad = R.pad_rule(tri_v)
    rec, lo, hi = R.tri_records(order, tri_v)
    out = dict(pad=pad, order=order, tris=rec, codes=codes, nodes8=None, off8=None, need8=0, depth8=0)
    for w in widths:
        t = wide_tree(keys, max_leaf, w)
        out[f"nodes{w}"] = R.refit_nodes(t["nodes"], w, lo, hi, pad)
        out[f"off{w}"], out[f"need{w}"], out[f"depth{w}"] = t["off"], t["need"], t["depth"]
    out["nodes4q"] = R.quantize4(out["nodes4"], pad)
    return out


# ------------------------------------------------------------------ hostile shapes
def one_triangle():
    return np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)


def grid(n, z=0.25):
    """n x n quads (2 n^2 triangles) in the plane z."""
    t = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (i, j, z), (i + 1, j, z), (i + 1, j + 1, z), (i, j + 1, z)
            t += [a + b + c, a + c + d]
    return np.array(t, np.float32)


def edge_case(first_scene_tri_v, name):
    """The hostile shapes of DESIGN.md §14 as (n, 9) triangles; `duplicates` repeats the first triangle given."""
    if name == "none":
        return np.zeros((0, 9), np.float32)
    if name == "one":
        return one_triangle()
    if name == "three":
        return grid(2)[:3]
    if name == "duplicates":
        return np.tile(np.asarray(first_scene_tri_v, F).reshape(-1, 9)[:1], (300, 1))
    if name == "same-centroid":       # triangles of growing size about one centre
        s = np.arange(1, 101, dtype=np.float32)[:, None]
        z = 0 * s
        return np.concatenate([-s, -s, z, s, -s, z, z, s, z], 1)      # bounds (-s, -s, 0) .. (s, s, 0)
    if name == "plane":
        return grid(9)
    raise KeyError(name)


# ------------------------------------------------------------------ checks
def leaf_cover(nodes, width, n_slots, max_leaf):
    """(slots not in exactly one leaf, leaves over max_leaf slots)."""
    refs = R.refs_of(nodes, width)
    seen = np.zeros(n_slots, np.int64)
    over = 0
    for r in refs[(refs < 0)]:
        v = -int(r) - 1
        first, count = v >> 3, (v & 7) + 1
        seen[first:first + count] += 1
        over += count > max_leaf
    return int((seen != 1).sum()), int(over)


def numbering(nodes, width, off):
    """(children not numbered above their parent, inner children outside the level right below their parent's,
    nodes that no parent or more than one names)."""
    refs = R.refs_of(nodes, width)
    level = np.searchsorted(off, np.arange(nodes.shape[0]), side="right") - 1
    named = np.zeros(nodes.shape[0], np.int64)
    low = skip = 0
    for i in range(nodes.shape[0]):
        for r in refs[i]:
            if r < 0 or r == EMPTY:
                continue
            low += r <= i
            skip += level[r] != level[i] + 1
            named[r] += 1
    return int(low), int(skip), int((named[1:] != 1).sum() + (named[0] != 0))


def walked_need(nodes, width):
    """The stack entries a depth-first walk can hold: one sentinel, at each visit one entry per child but the one
    it continues with, and the width - 1 slots a visit writes above the top."""
    refs = R.refs_of(nodes, width)
    most, stack = 0, [(0, 0)]
    while stack:
        i, held = stack.pop()
        most = max(most, held)
        live = [int(r) for r in refs[i] if r != EMPTY]
        for r in live:
            if r >= 0:
                stack.append((r, held + len(live) - 1))
    return 1 + most + width - 1

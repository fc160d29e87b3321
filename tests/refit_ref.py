"""NumPy restatement of the device refit of a resident scene (pyrenderer_amd/csrc/prt_refit.hip):
from the tree the host built (`Bvh(...).export()`'s order, `Bvh.collapse(4 | 8)`'s nodes), the pad rule and
new vertices to the triangle records, the refit wide nodes and the quantised four-wide nodes, word for word;
and the containment checks a refit tree has to pass.  Pure NumPy, every f32 step kept in f32.

Layouts (include/prt.h prt_bvh_collapse): a wide node holds its children in groups of four, plane p (lo.x,
hi.x, lo.y, hi.y, lo.z, hi.z) of child k at float (k // 4) * 24 + 4 p + k % 4, the child refs (int32 bits)
after the last group; an empty slot has lo = +inf, hi = -inf, ref = 0x7FFFFFFF; a leaf ref is
-(first * 8 + count - 1) - 1."""
import numpy as np

F = np.float32
EMPTY = 0x7FFFFFFF


def pad_rule(tri_v):
    """The builder's box padding for these vertices: max(largest |coordinate|, largest extent) * 1e-6f + 1e-30f."""
    v = np.asarray(tri_v, F).reshape(-1, 3)
    if v.shape[0] == 0:
        return F(1e-30)
    big = max(F(np.abs(v).max()), F((v.max(0) - v.min(0)).max()))
    return F(F(big * F(1e-6)) + F(1e-30))


def tri_records(order, tri_v):
    """(records (n_slots, 12), lo (n_slots, 3), hi (n_slots, 3)): slot s holds triangle order[s] as (v0, id bits)
    (v1 - v0, 0) (v2 - v0, 0), and the bounds of its three vertices."""
    order = np.asarray(order, np.int32)
    t = np.asarray(tri_v, F).reshape(-1, 3, 3)[order]
    rec = np.zeros((order.shape[0], 12), F)
    rec[:, 0:3] = t[:, 0]
    rec[:, 3] = order.view(F)
    rec[:, 4:7] = t[:, 1] - t[:, 0]
    rec[:, 8:11] = t[:, 2] - t[:, 0]
    return rec, t.min(1), t.max(1)


def refs_of(nodes, width):
    return np.ascontiguousarray(nodes[:, 6 * width:7 * width]).view(np.int32)


def plane(k, p):
    return (k // 4) * 24 + 4 * p + k % 4


def child_boxes(node, width):
    """(lo (width, 3), hi (width, 3)) of one node record."""
    lo = np.array([[node[plane(k, 2 * a)] for a in range(3)] for k in range(width)], F)
    hi = np.array([[node[plane(k, 2 * a + 1)] for a in range(3)] for k in range(width)], F)
    return lo, hi


def refit_nodes(nodes, width, lo, hi, pad):
    """The wide tree `nodes` refit to the slot bounds (lo, hi): a leaf child's box is the union of its slots'
    bounds, lo - pad and hi + pad in f32; an inner child's the union of the non-empty child boxes of the node
    it names.  A child is numbered above its parent, so the nodes go last to first.  Refs and empty slots stay."""
    out = np.array(nodes, F, copy=True)
    refs = refs_of(out, width)
    pad = F(pad)
    for i in range(out.shape[0] - 1, -1, -1):
        for k in range(width):
            r = int(refs[i, k])
            if r == EMPTY:
                continue
            if r < 0:
                v = -r - 1
                first, count = v >> 3, (v & 7) + 1
                blo = (lo[first:first + count].min(0) - pad).astype(F)
                bhi = (hi[first:first + count].max(0) + pad).astype(F)
            else:
                assert r > i, (i, k, r)
                clo, chi = child_boxes(out[r], width)
                live = refs[r] != EMPTY
                blo, bhi = clo[live].min(0), chi[live].max(0)
            for a in range(3):
                out[i, plane(k, 2 * a)] = blo[a]
                out[i, plane(k, 2 * a + 1)] = bhi[a]
    return out


def _round_down(x):
    f = x.astype(F)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, F(-np.inf)), f).astype(F)


def _round_up(x):
    f = x.astype(F)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, F(np.inf)), f).astype(F)


def quantize4(nodes4, pad):
    """quantize_bvh4 (prt_bvh_util.h quantize_node4) on (n, 32) four-wide nodes: (n, 16) f32 words.  Per axis the
    origin = the f32 at or below lo - 2 pad, the step = the f32 at or above (hi + 2 pad - origin) / 254 (and
    >= 1e-30), the child planes floor / ceil on that grid, clamped to 0..255, one byte per child."""
    n4 = np.asarray(nodes4, F)
    n = n4.shape[0]
    q = np.zeros((n, 16), F)
    qi = q.view(np.uint32)
    margin = 2.0 * float(F(pad))
    ok = np.isfinite(n4[:, 0:4])
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            l = n4[:, 8 * a:8 * a + 4].astype(np.float64)
            h = n4[:, 8 * a + 4:8 * a + 8].astype(np.float64)
            lo = np.where(ok, l, np.inf).min(1)
            hi = np.where(ok, h, -np.inf).max(1)
            none = ~(lo <= hi)
            lo, hi = np.where(none, 0.0, lo), np.where(none, 0.0, hi)
            o = _round_down(lo - margin)
            ext = hi + margin - o.astype(np.float64)
            st = np.maximum(_round_up(ext / 254.0), F(1e-30)).astype(F)
            q[:, a], q[:, 3 + a] = o, st
            o64, st64 = o.astype(np.float64)[:, None], st.astype(np.float64)[:, None]
            ql = np.clip(np.floor((np.where(ok, l, 0.0) - margin - o64) / st64), 0, 255).astype(np.uint32)
            qh = np.clip(np.ceil((np.where(ok, h, 0.0) + margin - o64) / st64), 0, 255).astype(np.uint32)
            ql, qh = np.where(ok, ql, 0).astype(np.uint32), np.where(ok, qh, 0).astype(np.uint32)
            shift = (8 * np.arange(4, dtype=np.uint32))[None]
            qi[:, 6 + 2 * a] = (ql << shift).sum(1, dtype=np.uint32)
            qi[:, 7 + 2 * a] = (qh << shift).sum(1, dtype=np.uint32)
    qi[:, 12:16] = np.where(ok, n4[:, 24:28].view(np.uint32), np.uint32(EMPTY))
    return q


def refit(order, nodes4, nodes8, tri_v):
    """Everything the device rewrites, from the creation-time tree and new vertices: dict(pad, tris, nodes4,
    nodes4q, nodes8); nodes8 None in, None out."""
    pad = pad_rule(tri_v)
    rec, lo, hi = tri_records(order, tri_v)
    n4 = refit_nodes(nodes4, 4, lo, hi, pad)
    n8 = None if nodes8 is None else refit_nodes(nodes8, 8, lo, hi, pad)
    return dict(pad=pad, tris=rec, nodes4=n4, nodes4q=quantize4(n4, pad), nodes8=n8)


# ------------------------------------------------------------------ checks
def planes_outside(refit_n, built_n, width):
    """Child planes of `refit_n` that lie strictly inside the built tree's (same topology): a count, 0 for a
    refit that is never tighter than the build."""
    live = refs_of(built_n, width) != EMPTY
    bad = 0
    for k in range(width):
        for a in range(3):
            m = live[:, k]
            bad += int((refit_n[m, plane(k, 2 * a)] > built_n[m, plane(k, 2 * a)]).sum())
            bad += int((refit_n[m, plane(k, 2 * a + 1)] < built_n[m, plane(k, 2 * a + 1)]).sum())
    return bad


def containment(nodes, width, order, tri_v, pad):
    """(triangles not inside their leaf's box with 0.9 pad to spare, child boxes not inside their parent's).
    The spare: a leaf plane is min - pad rounded to f32, an error of at most 2^-24 of a magnitude below
    1.000001 x the largest coordinate M, and pad >= 1e-6 M: 0.94 pad remains at the least."""
    refs = refs_of(nodes, width)
    tv = np.asarray(tri_v, np.float64).reshape(-1, 3, 3)[np.asarray(order)]
    spare = 0.9 * float(pad)
    loose_tri = loose_child = 0
    for i in range(nodes.shape[0]):
        lo, hi = child_boxes(nodes[i], width)
        for k in range(width):
            r = int(refs[i, k])
            if r == EMPTY:
                continue
            if r < 0:
                v = -r - 1
                t = tv[(v >> 3):(v >> 3) + (v & 7) + 1].reshape(-1, 3)
                loose_tri += int(((t - lo[k] < spare) | (hi[k] - t < spare)).any())
            else:
                clo, chi = child_boxes(nodes[r], width)
                live = refs[r] != EMPTY
                loose_child += int(((clo[live] < lo[k]) | (chi[live] > hi[k])).any())
    return loose_tri, loose_child


def displaced(tri_v, fraction=3, extents=0.5, axis=0):
    """tri_v with every `fraction`-th triangle translated along `axis` by `extents` of the scene's largest extent."""
    v = np.array(tri_v, F, copy=True).reshape(-1, 3, 3)
    p = v.reshape(-1, 3)
    v[::fraction, :, axis] += F(extents) * F((p.max(0) - p.min(0)).max())
    return v.reshape(-1, 9)

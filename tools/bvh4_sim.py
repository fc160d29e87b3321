"""While-while traversal of the Cornell BVH4 (octant front-to-back child order, as the LDS kernels'
octant copies) simulated on the CPU for waves of 64 extension rays (round 5, profiles/r05/coherence_sim/):
the leaf-buffering depth (npost: leaves a lane may hold before it stops descending; the kernels' "leaf +
cur" is 2) and the leaf-phase entry / exit thresholds (lb / le, the kernels' PRT_LEAF_BREAK / PRT_LEAF_EXIT),
priced with the per-trip VALU counts of the pooled kernel's ISA (79 per node visit, 73 per triangle test),
and the packed leaf trips of traverse_pk (every held leaf's triangles 64 to a trip).
--persistent (round 7, profiles/r07/pool_resume/): the pooled kernel's loop with suspended extension
tails.  A block of four waves runs in lockstep iterations: idle lanes take the next query of the block's
queue at the top of an iteration, the wave runs while-while rounds (npost 2, lb 0, le 8) and, after a
round, leaves the traversal if fewer than res_min lanes are still traversing and the queue still has
queries (the kernel's RES test); finished lanes shade and may enqueue a shadow ray (a uniform point of
the light, as the NEE sample), and the block's shadow rays go to the waves' free lanes (those without
a suspended query), one claim per wave.  Reported: E trips and lanes, iterations per 64 queries, the
share of iterations in which any lane shades, S trips with the free-lane claim against 64-ray chunks
of the same rays, and VALU per 64 queries with the iteration overhead priced per iteration.
The greedy collapse stands in for the build's SAH-optimal one (3.44 vs 3.17 node visits per query); at
npost 2 the lane fractions match the GPU lane table (0.463 / 0.269 against 0.444 / 0.294).

--width 8 (round 13, profiles/r13/lds_bvh8/): the same over the eight-wide tree of LDS-resident scenes (the
greedy collapse opened to 8 children, the octant orders over 8), a visit priced at the eight-wide visit's VALU
count (161 against 79 in the extension loop of the pooled kernel's listing; the shadow loop's 129 against 69
is not priced apart).  --le sweeps the leaf-phase exit of the plain table at npost 2, lb 0.

    python tools/bvh4_sim.py [--width {4,8}] [--le 8 16] [--persistent [--blocks 8] [--queries 2560]]
"""
import numpy as np, sys, time
sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__))))
from tools.coherence_sim import bounce_rays  # noqa: E402
from pyrenderer_amd import scenes
from pyrenderer_amd.io_utils.read_tungsten import read_file
from pyrenderer_amd.flatten import flatten_scene
from pyrenderer_amd._native import Bvh
SENT = 1 << 30

V_NODE_BY_WIDTH = {4: 79, 8: 161}   # VALU per node visit (E loop of the pooled kernel's listing: 77 and 159 in the visit's block, 2 around it)
V_TRI = 73
V_ITER_W4 = 539   # --persistent: VALU per wave iteration outside the traversals, as width 4's threshold-0 row calibrates it

def load(max_leaf=4, width=4):
    scene, cam = read_file(scenes.CORNELL)
    flat = flatten_scene(scene)
    nodes, tris, _ = Bvh(flat.tri_v, max_leaf=max_leaf).export()
    refs = nodes[:, 12:14].astype(np.float32).view(np.int32)
    def child(n, s):
        f = nodes[n, 6 * s:6 * s + 6].astype(np.float64)
        return (np.array([f[0], f[2], f[4]]), np.array([f[1], f[3], f[5]]), int(refs[n, s]))
    def area(c):
        d = c[1] - c[0]; return 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])
    # greedy collapse to `width` children
    n4 = []          # list of children lists
    def make(n2):
        ch = [child(n2, 0), child(n2, 1)]
        while len(ch) < width:
            inner = [i for i, c in enumerate(ch) if c[2] >= 0]
            if not inner: break
            i = max(inner, key=lambda i: area(ch[i]))
            c = ch.pop(i); ch += [child(c[2], 0), child(c[2], 1)]
        me = len(n4); n4.append(None)
        out = []
        for c in ch:
            if c[2] >= 0: out.append((c[0], c[1], make(c[2])))
            else: out.append(c)
        n4[me] = out
        return me
    make(0)
    # octant orders
    orders = []
    for ch in n4:
        o8 = []
        for k in range(8):
            def key(c):
                s = 0.0
                for ax in range(3):
                    s += -c[1][ax] if (k >> ax) & 1 else c[0][ax]
                return s
            o8.append(sorted(range(len(ch)), key=lambda i: (key(ch[i]), i)))
        orders.append(o8)
    T = tris.reshape(-1, 3, 4).astype(np.float64)
    return flat, cam, n4, orders, T

class Sim:
    def __init__(self, n4, orders, T):
        self.n4, self.orders, self.T = n4, orders, T
    def hitbox(self, c, o, inv, tmax):
        t0 = (c[0] - o) * inv; t1 = (c[1] - o) * inv
        tn = max(np.max(np.minimum(t0, t1)), 1e-5); tf = min(np.min(np.maximum(t0, t1)), tmax)
        return tn <= tf
    def tri(self, k, o, d, best):
        v0, e1, e2 = self.T[k, 0, :3], self.T[k, 1, :3], self.T[k, 2, :3]
        c = np.cross(e1, d); det = c @ e2
        if det == 0: return None
        f = 1.0 / det; s = o - v0; q = np.cross(s, e2)
        t, u, v = -f * (q @ e1), -f * (q @ d), f * (c @ s)
        return t if (1e-5 < t < best and u >= 0 and v >= 0 and 1 - u - v >= 0) else None
    def visit(self, j, st):
        o, d, inv, anyq = st['o'][j], st['d'][j], st['inv'][j], st['any'][j]
        k = int(d[0] < 0) | (int(d[1] < 0) << 1) | (int(d[2] < 0) << 2)
        ch = self.n4[st['cur'][j]]
        order = self.orders[st['cur'][j]][k]
        hits = [ch[i][2] for i in order if self.hitbox(ch[i], o, inv, st['best'][j])]
        if anyq: hits = hits[::-1]
        if hits:
            st['cur'][j] = hits[0]
            for r in reversed(hits[1:]): st['stk'][j].append(r)
        else:
            st['cur'][j] = st['stk'][j].pop()

    @staticmethod
    def state(n):
        return {'o': [None]*n, 'd': [None]*n, 'inv': [None]*n, 'best': [0.0]*n, 'any': [False]*n, 'hit': [-1]*n,
                'cur': [SENT]*n, 'leaves': [[] for _ in range(n)], 'stk': [[SENT] for _ in range(n)], 'qi': [0]*n}
    @staticmethod
    def start(st, j, q):
        st['o'][j], st['d'][j], st['best'][j], st['any'][j] = q
        st['inv'][j] = 1.0 / np.where(q[1] == 0, 1e-30, q[1])
        st['cur'][j], st['leaves'][j], st['stk'][j], st['hit'][j] = 0, [], [SENT], -1
    @staticmethod
    def active(st, j): return not (st['cur'][j] == SENT and not st['leaves'][j])

    def round(self, st, lb=0, le=8, npost=1, packed=False):
        """One outer while-while round (inner phase, then leaf phase) of the wave's lanes:
        (inner trips, inner lanes, triangle trips, triangle lanes, leaf rounds)."""
        n = len(st['cur'])
        wi = li = wl = ll = rounds = 0
        while True:
            lanes = [j for j in range(n) if st['cur'][j] >= 0 and st['cur'][j] != SENT and len(st['leaves'][j]) < npost]
            if not lanes: break
            wi += 1; li += len(lanes)
            for j in lanes:
                self.visit(j, st)
                while st['cur'][j] != SENT and st['cur'][j] < 0 and len(st['leaves'][j]) < npost:
                    st['leaves'][j].append(st['cur'][j]); st['cur'][j] = st['stk'][j].pop()
            if sum(1 for j in range(n) if st['cur'][j] >= 0 and st['cur'][j] != SENT and not st['leaves'][j]) <= lb: break
        while True:
            lanes = [j for j in range(n) if st['leaves'][j]]
            if not lanes: break
            rounds += 1
            work = {}
            for j in lanes:
                tl = []
                for lf in st['leaves'][j]:
                    v = -lf - 1; tl += list(range(v >> 3, (v >> 3) + (v & 7) + 1))
                work[j] = tl
            done_any = set()
            if packed:
                P = sum(len(w) for w in work.values())
                wl += -(-P // 64); ll += P
                for j in lanes:
                    b0 = st['best'][j]
                    ts = [t for t in (self.tri(k, st['o'][j], st['d'][j], b0) for k in work[j]) if t is not None]
                    if ts:
                        st['best'][j] = min(ts)
                        if st['any'][j]: done_any.add(j)
            for k in range(0 if packed else max(len(w) for w in work.values())):
                act = [j for j in lanes if k < len(work[j]) and j not in done_any]
                if not act: break
                wl += 1; ll += len(act)
                for j in act:
                    t = self.tri(work[j][k], st['o'][j], st['d'][j], st['best'][j])
                    if t is not None:
                        st['best'][j] = t; st['hit'][j] = work[j][k]
                        if st['any'][j]: done_any.add(j)
            for j in lanes:
                st['leaves'][j] = []
                if j in done_any: st['cur'][j] = SENT; continue
                while st['cur'][j] != SENT and st['cur'][j] < 0 and len(st['leaves'][j]) < npost:
                    st['leaves'][j].append(st['cur'][j]); st['cur'][j] = st['stk'][j].pop()
            if sum(1 for j in range(n) if st['leaves'][j]) <= le: break
        return wi, li, wl, ll, rounds

    def wave(self, queries, lb=0, le=8, npost=1, packed=False):
        """Trip counts of one wave: (inner trips, inner lanes, triangle trips, triangle lanes, leaf rounds).
        packed: a leaf round tests the (lane, triangle) pairs of every held leaf 64 to a trip
        (traverse_pk, round 5) against each lane's bound at the round's start."""
        n = len(queries)
        st = self.state(n)
        tot = np.zeros(5, np.int64)
        while True:
            for j in range(n):
                if not self.active(st, j) and st['qi'][j] < len(queries[j]):
                    self.start(st, j, queries[j][st['qi'][j]]); st['qi'][j] += 1
            if not any(self.active(st, j) for j in range(n)): break
            tot += self.round(st, lb, le, npost, packed)
        return tuple(int(x) for x in tot)

    def block(self, queue, thr, shadow, waves=4, lb=0, le=8, npost=2):
        """trace_kernel_pool's loop for one block of `waves` waves over the block's `queue` of extension
        queries.  thr: a wave leaves its traversal after a round once at most thr lanes are still
        traversing and the queue is not empty (TraceParams::pool_resume_min; 0: never).
        shadow(o, d, t, tri) -> any-hit query of the finished lane, or None.  Returns a dict of counts."""
        sts = [self.state(64) for _ in range(waves)]
        nxt = 0
        E = np.zeros(5, np.int64); Sf = np.zeros(5, np.int64); Sc = np.zeros(5, np.int64)
        c = dict(iters=0, shade_iters=0, finished=0, suspended=0, shadow=0, block_iters=0)
        while True:
            pool, free, ran = [], [], False
            for st in sts:
                for j in range(64):
                    if not self.active(st, j) and nxt < len(queue):
                        self.start(st, j, queue[nxt]); nxt += 1
                was = [j for j in range(64) if self.active(st, j)]
                if not was:
                    free.append(64)
                    continue
                c['iters'] += 1; ran = True
                while True:
                    E += self.round(st, lb, le, npost)
                    act = sum(1 for j in was if self.active(st, j))
                    if act == 0 or (act <= thr and nxt < len(queue)): break
                fin = [j for j in was if not self.active(st, j)]
                c['shade_iters'] += 1 if fin else 0
                c['finished'] += len(fin); c['suspended'] += len(was) - len(fin)
                free.append(64 - (len(was) - len(fin)))
                for j in fin:
                    q = shadow(st['o'][j], st['d'][j], st['best'][j], st['hit'][j])
                    if q is not None: pool.append(q)
            if not ran: break
            c['block_iters'] += 1
            c['shadow'] += len(pool)
            # S: the queue's rays to the waves' free lanes, one claim per wave, against 64-ray chunks
            e = 0
            for f in free:
                if e >= len(pool): break
                Sf += self.wave([[q] for q in pool[e:e + f]], lb, le, npost)
                e += f
            for e in range(0, len(pool), 64):
                Sc += self.wave([[q] for q in pool[e:e + 64]], lb, le, npost)
        c.update(E=E, S_free=Sf, S_chunk=Sc, queries=len(queue))
        return c


def persistent(args):
    """The --persistent table (see the module docstring)."""
    flat, cam, n4, orders, T = load(width=args.width)
    sim = Sim(n4, orders, T)
    rng = np.random.default_rng(0)
    O_, D_, B = bounce_rays(flat, cam, 20000, rng)
    nq = args.blocks * args.queries
    perm = rng.permutation(len(O_))[:nq]
    # NEE sample of a finished lane: a uniform point of the light's triangles, queried when both cosines are
    # positive (the light faces down); hits on the light itself end the path
    tv = flat.tri_v.reshape(-1, 3, 3).astype(np.float64)
    lt = tv[flat.light_tri]
    tri_id = np.ascontiguousarray(T[:, 0, 3].astype(np.float32)).view(np.int32)
    light_ids = set(int(i) for i in flat.light_tri)
    def shadow(o, d, t, k):
        if k < 0 or int(tri_id[k]) in light_ids: return None
        p = o + d * t
        n = np.cross(T[k, 1, :3], T[k, 2, :3]); n /= np.linalg.norm(n)
        if n @ d > 0: n = -n
        L = lt[rng.integers(len(lt))]
        su, sv = np.sqrt(rng.random()), rng.random()
        p2 = L[0] * (su * (1 - sv)) + L[1] * (su * sv) + L[2] * (1 - su)
        w = p2 - p; dist = np.linalg.norm(w); w /= dist
        if not (n @ w > 0 and w[1] > 0): return None
        return (p, w, dist, True)
    # VALU per trip from the pooled kernel's ISA; the rest of an iteration (shading, S claim, resolve, refill,
    # loop control) is priced per wave iteration, calibrated on the threshold-0 row so that E : (S + rest) is
    # the profiled 102 : 96 wave-level VALU per sample
    V_NODE = V_NODE_BY_WIDTH[args.width]
    print(f"persistent model: width {args.width} ({len(n4)} nodes, {V_NODE} VALU per visit), {args.blocks} blocks x "
          f"{args.queries} queries, 4 waves, npost 2 lb 0 le {args.le[0]}")
    print("thr | E node trips/64q (lanes) | E tri trips/64q (lanes) | iter/64q | shade share | susp/query | "
          "S node+tri trips/64q free-lane (lanes n, t) | same rays in 64-chunks | VALU/64q E, S, iter, total")
    rows = []
    for thr in args.thresholds:
        tot = None
        for b in range(args.blocks):
            queue = [(O_[i], D_[i], 99999.9, False) for i in perm[b * args.queries:(b + 1) * args.queries]]
            r = sim.block(queue, thr, shadow, le=args.le[0])
            if tot is None: tot = r
            else:
                for k, v in r.items(): tot[k] = tot[k] + v
        rows.append((thr, tot))
        print(f"# threshold {thr} done", file=sys.stderr, flush=True)
    # width 8 takes the rest of an iteration as calibrated at width 4 (the profiled ratio is that build's)
    v_iter = None if args.width == 4 else V_ITER_W4
    if v_iter is not None:
        print(f"rest of an iteration: {v_iter:.0f} VALU per wave iteration (the width-4 calibration)")
    for thr, tot in rows:
        w = tot['queries'] / 64.0
        E, Sf, Sc = tot['E'], tot['S_free'], tot['S_chunk']
        ve = (E[0] * V_NODE + E[2] * V_TRI) / w
        vs = (Sf[0] * V_NODE + Sf[2] * V_TRI) / w
        if v_iter is None:   # the first row (threshold 0) calibrates the per-iteration rest
            v_iter = (ve * 96.0 / 102.0 - vs) / (tot['iters'] / w)
            print(f"rest of an iteration: {v_iter:.0f} VALU per wave iteration")
        vi = tot['iters'] * v_iter / w
        print(f"{thr:3d} | {E[0]/w:5.2f} ({E[1]/(64*E[0]):.3f}) | {E[2]/w:5.2f} ({E[3]/(64*E[2]):.3f}) | "
              f"{tot['iters']/w:.3f} | {tot['shade_iters']/tot['iters']:.3f} | {tot['suspended']/tot['queries']:.3f} | "
              f"{Sf[0]/w:5.2f} + {Sf[2]/w:5.2f} ({Sf[1]/(64*max(Sf[0],1)):.3f}, {Sf[3]/(64*max(Sf[2],1)):.3f}) | "
              f"{Sc[0]/w:5.2f} + {Sc[2]/w:5.2f} | {ve:.0f}, {vs:.0f}, {vi:.0f}, {ve+vs+vi:.0f}", flush=True)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--persistent", action="store_true", help="the pooled kernel's loop with suspended extension tails")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--queries", type=int, default=2560, help="extension queries per block")
    ap.add_argument("--thresholds", type=int, nargs="+", default=[0, 7, 11, 15, 23, 31])
    ap.add_argument("--width", type=int, choices=(4, 8), default=4, help="children per node of the collapsed tree")
    ap.add_argument("--le", type=int, nargs="+", default=None,
                    help="leaf-phase exit thresholds: the plain table's sweep at npost 2, lb 0 (instead of its "
                         "full grid); --persistent takes the first (default 8)")
    args = ap.parse_args()
    sweep = args.le
    args.le = args.le or [8]
    if args.persistent:
        persistent(args)
        sys.exit(0)
    flat, cam, n4, orders, T = load(width=args.width)
    V_NODE = V_NODE_BY_WIDTH[args.width]
    print(f"BVH{args.width} nodes", len(n4), "| VALU per visit", V_NODE)
    sim = Sim(n4, orders, T)
    rng = np.random.default_rng(0)
    O_, D_, B = bounce_rays(flat, cam, 20000, rng)
    perm = rng.permutation(len(O_))[:64 * 150]
    def run(label, X=30, Y=25, **kw):
        """X / Y: extra VALU per packed trip (owner scan, (t, id) reduction) / per packed round (prefix sums)"""
        wi = li = wl = ll = rr = 0
        for g in range(0, len(perm), 64):
            r = sim.wave([[(O_[i], D_[i], 99999.9, False)] for i in perm[g:g + 64]], **kw)
            wi, li, wl, ll, rr = wi + r[0], li + r[1], wl + r[2], ll + r[3], rr + r[4]
        nq = len(perm)
        pk = kw.get("packed", False)
        cost = (wi * V_NODE + wl * (V_TRI + (X if pk else 0)) + (rr * Y if pk else 0)) / (nq / 64)
        print(f"{label:28s} inner trips/wave {wi/(nq/64):.2f} lanes {li/(64*wi):.3f} | tri trips/wave {wl/(nq/64):.2f} lanes {ll/(64*wl):.3f} | visits/ray {li/nq:.2f} tests/ray {ll/nq:.2f} | VALU/wave {cost:.0f}", flush=True)
    print("---")
    if sweep:
        for le in sweep:
            run(f"npost 2 lb0 le{le}", npost=2, lb=0, le=le)
        sys.exit(0)
    for npost in (2, 3, 4):
        for lb, le in ((0, 8), (4, 8), (8, 8), (0, 16), (8, 16)):
            run(f"npost {npost} lb{lb} le{le}", npost=npost, lb=lb, le=le)
    print("--- packed leaf trips (traverse_pk): 30 extra VALU per trip, 25 per round")
    for npost in (1, 2, 3, 4):
        for lb, le in ((0, 0), (0, 8), (4, 8)):
            run(f"packed npost {npost} lb{lb} le{le}", npost=npost, lb=lb, le=le, packed=True)

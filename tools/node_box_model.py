"""CPU model of the lattice packet walk with the NODE BOXES (mesh_rules.h: range_box_setup / node_box_make; geom_device.h:
nearest_packet): a parent whose two children both hold at most N triangles tests them by one oriented box each instead of their
AABBs.  Everything above such parents stays AABB, the leaves keep their pair boxes.

Built on tools/pair_box_model.py (tree, float64 distances, packets); its results are not touched.  The committed rule
(N = kNodeBoxMaxTris = 16) is read from the host builder's arena - the records the GPU walks on; the other thresholds of the
table restate the rule in float64 numpy.  Every variant must find the same 64 (d^2, face) keys per packet as the walk without
node boxes: asserted.

    python tools/node_box_model.py --mesh body --res 257 --packets 250 --seed 1
    python tools/node_box_model.py --mesh body --res 65 --packets 0 --thresholds 16     # every packet: the GPU's counters

Estimated VALU instructions per packet, counted in the compiled loop of k_nearest<lattice> with "box_clamp" on
(profiles/walk_diet_isa.txt) = 20 per AABB node visit (15 box + 2 votes, ~3 of push / pop per visit) + 26 per oriented node visit
(21 of pair_box_bound_half + 2 votes, the same ~3) + 24 per leaf visit (21 + 2, the bound update of a tested leaf) + 61 per pair
tested (51 distance + 10 key update) + 70 of set-up; dependent load rounds = node visits + leaf visits.  The GPU's counters for the same walk: tools/trav_stats.py (MeshHandle.walk_stats).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_box_model as pbm  # noqa: E402

K_MAX_TRIS = 16                 # mesh_rules.h: kNodeBoxMaxTris
K_FLAG = 1 << 30                # mesh_rules.h: kNodeBoxFlag
K_SCALE, K_EPS, K_FLOOR = np.float64(np.float32(0.9999)), np.float64(np.float32(4e-6)), np.float64(np.float32(1e-15))


class NodeTree(pbm.Tree):
    """pair_box_model.Tree plus the node-box section of the arena, the walk references of the nodes and every node's slot range"""

    def __init__(self, v, f):
        super().__init__(v, f)
        v = np.ascontiguousarray(v, np.float32); f = np.ascontiguousarray(f, np.int64)
        F = self.F
        lay, ar = pbm.host_arena(v, f)
        up = lambda n: (n + 255) // 256 * 256
        nb_at = lay[3] + up(384 * F) + up(128 * F)                        # leaves, pair boxes, node boxes
        assert nb_at + up(128 * F) == lay[4], "arena layout: the node boxes end where the triangle records begin"
        self.nbox = ar[nb_at:nb_at + 128 * F].view(np.float32).reshape(F, 16, 2).copy()
        self.pbox64 = self.pbox.astype(np.float64)
        self.walk_child = ar[lay[2]:lay[2] + 64 * F].view(np.int32).reshape(F, 16)[:, 14:16].copy()
        self.begin, self.end = np.zeros(F, np.int64), np.zeros(F, np.int64)
        self.is_node = np.zeros(F, bool)

        def span(r):
            if r < 0:
                leaf, cnt = (~r) >> 2, ((~r) & 3) + 1
                return leaf, leaf + cnt
            b, m0 = span(int(self.child[r, 0])); m1, e = span(int(self.child[r, 1]))
            assert m0 == m1 == r + 1, "node id = split point - 1, contiguous slot ranges"
            self.begin[r], self.end[r], self.is_node[r] = b, e, True
            return b, e
        sys.setrecursionlimit(10000)
        self.span = span(self.root)

    def oriented(self, n_max):
        """bool [F]: the inner nodes whose children both hold at most n_max triangles"""
        ids = np.arange(self.F)
        return self.is_node & (ids + 1 - self.begin <= n_max) & (self.end - (ids + 1) <= n_max)

    def arena_boxes(self):
        """(oriented [F] bool, rec [F,16,2] f64) as the builder committed them"""
        return self.nbox[:, 3:12].any((1, 2)), self.nbox.astype(np.float64)

    def model_boxes(self, n_max):
        """the same for another threshold: the rule restated in float64"""
        op = self.oriented(n_max)
        rec = np.zeros((self.F, 16, 2))
        for r in np.nonzero(op)[0]:
            rec[r, :15, 0] = range_box64(self.tri[self.begin[r]:r + 1])
            rec[r, :15, 1] = range_box64(self.tri[r + 1:self.end[r]])
        return op, rec


def range_box64(tri):
    """float64 restatement of range_box_setup for tri [n,3,3] -> the 15 fields"""
    t = np.asarray(tri, np.float64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    e = np.stack([b - a, c - a, c - b], 1)                                # [n, 3 edges, 3]
    l2 = (e * e).sum(-1).reshape(-1)
    best = int(np.argmax(l2))                                             # the first maximum in (slot, edge) order
    L2, eb = l2[best], e.reshape(-1, 3)[best]
    n = np.cross(e[:, 0], e[:, 1]).sum(0)
    ax = np.eye(3)
    nn = n @ n
    if nn > 1e-10 * L2 * L2:
        a0 = n / np.sqrt(nn)
        u = eb - (eb @ a0) * a0
        if u @ u > 1e-10 * L2:
            a1 = u / np.sqrt(u @ u)
            ax = np.stack([a0, a1, np.cross(a0, a1)])
    pts = t.reshape(-1, 3)
    c0 = 0.5 * (pts.min(0) + pts.max(0))
    pr = (pts - c0) @ ax.T
    c0 = c0 + (0.5 * (pr.min(0) + pr.max(0))) @ ax
    sax = ax * K_SCALE
    h = np.abs((pts - c0) @ sax.T).max(0)
    return np.concatenate([c0, sax.reshape(-1), h + (K_EPS * h.sum() + K_FLOOR)])


class WalkArrays:
    """the tree as float64 arrays indexed by node / leaf id, for walk_many"""

    def __init__(self, tree, boxes):
        F = tree.F
        self.root, self.child = tree.root, tree.child.astype(np.int64)
        self.lo, self.hi = tree.lo[:, None], tree.hi[:, None]             # [F, 1, axis, child]
        self.op = np.zeros(F, bool) if boxes is None else boxes[0]
        rec = np.zeros((F, 16, 2)) if boxes is None else boxes[1]
        split = lambda r: (r[:, 0:3].transpose(0, 2, 1)[:, None], r[:, 3:12].reshape(-1, 3, 3, 2).transpose(0, 3, 1, 2),
                           r[:, 12:15].transpose(0, 2, 1)[:, None])        # centre [F,1,c,xyz], axes [F,c,axis,xyz], half extents [F,1,c,axis]
        self.nb, self.pb = split(rec), split(tree.pbox64)
        slot = np.minimum(np.arange(F)[:, None] + np.arange(4)[None], np.arange(F)[:, None] + np.maximum(tree.leaf_cnt, 1)[:, None] - 1)
        slot = np.minimum(slot, F - 1)
        self.tri4 = tree.tri[slot].astype(np.float64)                     # [leaf id, 4, 3, 3]: short leaves repeat their last triangle
        self.face4 = tree.order[slot].astype(np.int64)


def _bound_many(box, ids, P):
    c, A, h = box
    t = np.einsum("glck,gcak->glca", P[:, :, None, :] - c[ids], A[ids])
    e = np.maximum(np.abs(t) - h[ids], 0.0)
    return (e * e).sum(-1)                                                # [g, 64, child]


def walk_many(tree, P, live, boxes=None, center=21):
    """pair_box_model.walk with the node boxes, for B packets in lockstep (P [B,64,3], live [B,64]; boxes = (oriented [F] bool,
    rec [F,16,2] f64), or None: AABBs only): every round each unfinished packet makes ONE visit - the packets at AABB nodes, at
    oriented parents and at leaves as three batches.  A packet's walk does not depend on the others'.
    Returns (counts summed over the packets, d2 [B,64], face [B,64]) - the key of every lane: the minimum of (d^2, face)."""
    W = boxes if isinstance(boxes, WalkArrays) else WalkArrays(tree, boxes)
    B = len(P)
    best = np.full((B, 64), np.inf); face = np.full((B, 64), 0x7fffffff, np.int64)
    thr = np.where(live, np.inf, -np.inf)
    cur = np.full(B, W.root, np.int64); sp = np.zeros(B, np.int64); stack = np.zeros((B, 64), np.int64)
    done = np.zeros(B, bool)
    st = dict(aabb=0, obox=0, leaves=0, offered=0, tested=0)

    def pop(g):                                                           # packets g take their next subtree from their stack, or finish
        empty = sp[g] == 0
        done[g[empty]] = True
        h = g[~empty]
        sp[h] -= 1
        cur[h] = stack[h, sp[h]]
    while not done.all():
        act = np.nonzero(~done)[0]
        at_leaf = cur[act] < 0
        g = act[at_leaf]
        if len(g):
            code = ~cur[g]
            L, cnt = code >> 2, (code & 3) + 1
            npairs = (cnt + 1) // 2
            need = (_bound_many(W.pb, L, P[g]) <= thr[g][:, :, None]).any(1) & (np.arange(2)[None] < npairs[:, None])
            st["leaves"] += len(g); st["offered"] += int(npairs.sum()); st["tested"] += int(need.sum())
            t = need.any(1)
            gt, Lt = g[t], L[t]
            if len(gt):
                d4 = pbm.tri_dist2(P[gt][:, :, None, :], W.tri4[Lt][:, None])         # [g, 64, 4]
                for s in range(4):
                    use = need[t][:, s >> 1] & (s < cnt[t])
                    d, fc = d4[:, :, s], W.face4[Lt, s][:, None]
                    better = use[:, None] & ((d < best[gt]) | ((d == best[gt]) & (fc < face[gt])))
                    best[gt] = np.where(better, d, best[gt]); face[gt] = np.where(better, fc, face[gt])
                thr[gt] = np.where(live[gt], pbm.prune_threshold(best[gt]), thr[gt])
            pop(g)
        at_node = act[~at_leaf]
        at_op = W.op[cur[at_node]]
        for oriented in (False, True):
            g = at_node[at_op == oriented]
            if not len(g):
                continue
            n = cur[g]
            if oriented:
                st["obox"] += len(g)
                d = _bound_many(W.nb, n, P[g])
            else:
                st["aabb"] += len(g)
                Pe = P[g][:, :, :, None]
                dd = np.maximum(np.maximum(W.lo[n] - Pe, Pe - W.hi[n]), 0.0)
                d = (dd * dd).sum(2)
            v = (d <= thr[g][:, :, None]).any(1)
            first0 = d[:, center, 0] <= d[:, center, 1]
            c0, c1 = W.child[n, 0], W.child[n, 1]
            both = v[:, 0] & v[:, 1]
            gb = g[both]
            stack[gb, sp[gb]] = np.where(first0, c1, c0)[both]
            sp[gb] += 1
            cur[g] = np.where(both, np.where(first0, c0, c1), np.where(v[:, 0], c0, c1))
            pop(g[~v.any(1)])
    return st, best, face


def blocks_of(res, packets, seed):
    nb = (res + 3) // 4
    if packets and packets < nb ** 3:
        return np.random.RandomState(seed).randint(0, nb, (packets, 3))
    g = np.arange(nb)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def model(tree, res, blocks, variants):
    """variants: {name: boxes or None}; the first one is the reference whose keys all others must reproduce, lane for lane.
    Returns {name: mean counts per packet}"""
    packets = [pbm.lattice_packet(res, int(bx), int(by), int(bz)) for bx, by, bz in blocks]
    P, live = np.stack([p for p, _ in packets]), np.stack([l for _, l in packets])
    out, ref = {}, None
    for name, boxes in variants.items():
        st, d2, fc = walk_many(tree, P, live, boxes)
        if ref is None:
            ref = (d2, fc)
        else:
            bad = np.nonzero(((d2 != ref[0]) | (fc != ref[1])) & live)[0]
            assert len(bad) == 0, f"{name}: another key in packet {tuple(blocks[bad[0]])}"
        out[name] = {c: v / len(blocks) for c, v in st.items()}
    return out


def estimate(r):
    return 20 * r["aabb"] + 26 * r["obox"] + 24 * r["leaves"] + 61 * r["tested"] + 70


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", default="body")
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--packets", type=int, default=250, help="random 4^3 packets of the lattice (0: all of them)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresholds", default="8,16,32,64")
    a = ap.parse_args()
    v, f = pbm.mesh_by_name(a.mesh)
    tree = NodeTree(v, f)
    variants = {"off": None}
    for n in (int(x) for x in a.thresholds.split(",")):
        variants[f"{n} (arena)" if n == K_MAX_TRIS else str(n)] = tree.arena_boxes() if n == K_MAX_TRIS else tree.model_boxes(n)
    op = tree.oriented(K_MAX_TRIS)
    assert np.array_equal(op, tree.arena_boxes()[0]), "the arena's records are not exactly the oriented parents"
    r = model(tree, a.res, blocks_of(a.res, a.packets, a.seed), variants)
    print(f"mesh {a.mesh}, {a.res}^3 lattice, {len(blocks_of(a.res, a.packets, a.seed))} packets (seed {a.seed}); "
          f"{int(op.sum())} of {int(tree.is_node.sum())} inner nodes are oriented parents at N = {K_MAX_TRIS}; per 4^3 packet (mean):")
    print("| N | AABB node visits | oriented node visits | leaf visits | pairs offered | pairs tested | est. VALU | dependent load rounds |")
    print("|---|---|---|---|---|---|---|---|")
    for name, c in r.items():
        print(f"| {name} | {c['aabb']:.1f} | {c['obox']:.1f} | {c['leaves']:.1f} | {c['offered']:.1f} | {c['tested']:.1f} | {estimate(c):,.0f} | "
              f"{c['aabb'] + c['obox'] + c['leaves']:.1f} |")


if __name__ == "__main__":
    main()

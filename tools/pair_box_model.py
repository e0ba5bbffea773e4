"""CPU model of the lattice packet walk (icon_amd/csrc/geom_device.h: nearest_packet) on the project's REAL tree: where the
leaf work goes, and what the oriented pair boxes (PairBox, mesh_rules.h: pair_box_setup / pair_box_bound) remove from it.

The tree, the leaf order and the pair-box records are read from the arena of the host builder (icon_debug_host_mesh_build: no
GPU needed); the walk is restated in float64 numpy with the kernel's traversal order (near child first by the packet's centre
lane), its pruning bound and its parked lanes.  Per 4^3 packet it counts the nodes visited, the leaf pairs offered to the
distance test, the pairs that hold a triangle within reach of some lane (the ceiling of any pre-test) and the pairs that
survive the box test - the two numbers icon_debug_pair_stats (MeshHandle.pair_stats, tools/trav_stats.py) measures on the GPU.

    python tools/pair_box_model.py --mesh body --res 257 --packets 400 --seed 0
    python tools/pair_box_model.py --mesh body --res 65 --packets 0          # every packet: compare with the GPU's counters
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def host_arena(v, f, cm=None, vs=None):
    """(layout[12], arena bytes) of the host builder for the mesh (v [V,3] f32, f [F,3] i64)"""
    from icon_amd import _lib
    v = np.ascontiguousarray(v, np.float32); f = np.ascontiguousarray(f, np.int64)
    cm = np.zeros((len(v), 3), np.float32) if cm is None else np.ascontiguousarray(np.asarray(cm, np.float32).reshape(-1, 3))
    vs = np.zeros(len(v), np.float32) if vs is None else np.ascontiguousarray(np.asarray(vs, np.float32).reshape(-1))
    lay = (C.c_int64 * 12)()
    _lib.check(_lib.lib().icon_debug_mesh_layout(C.c_int64(len(v)), C.c_int64(len(f)), lay))
    lay = list(lay)
    ar = np.zeros(lay[11], np.uint8)
    _lib.check(_lib.lib().icon_debug_host_mesh_build(_lib.ptr(v), C.c_int64(len(v)), _lib.ptr(f), C.c_int64(len(f)), _lib.ptr(cm), _lib.ptr(vs),
                                                     _lib.ptr(ar), C.c_int64(len(ar))), "icon_debug_host_mesh_build")
    return lay, ar


class Tree:
    """the arena's search structures as numpy arrays"""

    def __init__(self, v, f):
        v = np.ascontiguousarray(v, np.float32); f = np.ascontiguousarray(f, np.int64)
        F = len(f)
        lay, ar = host_arena(v, f)
        self.F = F
        self.root = int(ar[lay[0]:lay[0] + 4].view(np.int32)[0])
        nodes = ar[lay[2]:lay[2] + 64 * F].view(np.float32).reshape(F, 16)
        self.lo = nodes[:, 0:6].reshape(F, 3, 2).astype(np.float64)       # [node][axis][child]
        self.hi = nodes[:, 6:12].reshape(F, 3, 2).astype(np.float64)
        self.child = nodes.view(np.int32)[:, 12:14].copy()
        self.order = ar[lay[6]:lay[6] + 4 * F].view(np.int32).copy()     # slot -> face
        self.tri = v[f[self.order]]                                       # [slot][corner][xyz] f32
        pb_at = lay[3] + (384 * F + 255) // 256 * 256                     # the pair boxes follow the leaf records
        self.pbox = ar[pb_at:pb_at + 128 * F].view(np.float32).reshape(F, 16, 2).copy()
        # leaves: walk the tree
        self.leaf_cnt = np.zeros(F, np.int32)
        stack = [self.root]
        while stack:
            r = stack.pop()
            if r < 0:
                self.leaf_cnt[(~r) >> 2] = ((~r) & 3) + 1
            else:
                stack += [int(self.child[r, 0]), int(self.child[r, 1])]

    def pairs(self):
        """every leaf pair: (leaf id [P], pair index [P], slot of its first / second triangle [P])"""
        leaf, pr, s0, s1 = [], [], [], []
        for L in np.nonzero(self.leaf_cnt)[0]:
            cnt = int(self.leaf_cnt[L])
            for p in range((cnt + 1) // 2):
                leaf.append(L); pr.append(p); s0.append(L + 2 * p); s1.append(L + min(2 * p + 1, cnt - 1))
        return np.array(leaf), np.array(pr), np.array(s0), np.array(s1)


def tri_dist2(p, tri):
    """float64 squared distance point - triangle, broadcasting p [..., 3] against tri [..., 3, 3] (closest point by regions,
    Ericson, Real-Time Collision Detection 5.1.5; zero-area triangles: the minimum over the three edges)"""
    p = np.asarray(p, np.float64); tri = np.asarray(tri, np.float64)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]

    def seg(o, e):
        ee = (e * e).sum(-1)
        t = np.clip(np.where(ee > 0, ((p - o) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
        d = p - o - t[..., None] * e
        return (d * d).sum(-1)
    ab, ac = b - a, c - a
    d_edge = np.minimum(np.minimum(seg(a, ab), seg(a, ac)), seg(b, c - b))
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    ap = p - a
    # barycentrics of the projection
    s = (np.cross(ap, ac) * n).sum(-1) / nn1
    t = (np.cross(ab, ap) * n).sum(-1) / nn1
    inside = ok & (s >= 0) & (t >= 0) & (s + t <= 1)
    h = (ap * n).sum(-1)
    d_face = h * h / nn1
    return np.where(inside, np.minimum(d_face, d_edge), d_edge)


def box_bound(rec, p):
    """float64 restatement of pair_box_bound: rec [..., 16] fields of ONE pair, p [..., 3]"""
    rec = np.asarray(rec, np.float64)
    d = np.asarray(p, np.float64) - rec[..., 0:3]
    out = 0.0
    for k in range(3):
        t = (rec[..., 3 + 3 * k:6 + 3 * k] * d).sum(-1)
        e = np.maximum(np.abs(t) - rec[..., 12 + k], 0.0)
        out = out + e * e
    return out


def prune_threshold(best):
    return best * np.float64(np.float32(1.000083)) + np.float64(np.float32(2.1e-7))


def walk(tree, P, live, center=21):
    """one packet: P [64,3] points, live [64] bool.  Returns a dict of counts."""
    best = np.full(64, np.inf)
    thr = np.where(live, np.inf, -np.inf)
    st = dict(nodes=0, leaves=0, offered=0, useful=0, boxed=0, leaves_boxed_out=0, leaves_useless=0, tris=0, tris_useful=0)
    stack, cur = [], tree.root
    while True:
        if cur < 0:
            code = ~cur
            L, cnt = code >> 2, (code & 3) + 1
            st["leaves"] += 1
            any_useful, any_boxed = False, False
            entry_thr = thr.copy()
            for pr in range((cnt + 1) // 2):
                s0, s1 = L + 2 * pr, L + min(2 * pr + 1, cnt - 1)
                d0 = tri_dist2(P, tree.tri[s0][None]); d1 = tri_dist2(P, tree.tri[s1][None])
                st["offered"] += 1
                st["tris"] += 2 if s1 != s0 else 1
                u0, u1 = bool((d0 <= entry_thr).any()), bool((d1 <= entry_thr).any())
                st["tris_useful"] += int(u0) + int(u1 and s1 != s0)
                useful = u0 or u1
                bb = box_bound(tree.pbox[L, :, pr], P)
                boxed = bool((bb <= entry_thr).any())              # (the kernel evaluates both boxes of a leaf at its entry)
                assert boxed or not bool((np.minimum(d0, d1) <= entry_thr).any()), "the box culled a pair a lane needs"
                st["useful"] += int(useful); st["boxed"] += int(boxed)
                any_useful |= useful; any_boxed |= boxed
                if boxed:                                     # (a culled pair cannot move any lane's best: skipping it changes nothing)
                    best = np.minimum(best, np.minimum(d0, d1))
                    thr = np.where(live, prune_threshold(best), thr)
            st["leaves_useless"] += int(not any_useful); st["leaves_boxed_out"] += int(not any_boxed)
            if not stack:
                break
            cur = stack.pop()
        else:
            st["nodes"] += 1
            lo, hi = tree.lo[cur], tree.hi[cur]                # [axis][child]
            dd = np.maximum(np.maximum(lo[None] - P[:, :, None], P[:, :, None] - hi[None]), 0.0)
            d = (dd * dd).sum(1)                               # [lane][child]
            v0, v1 = bool((d[:, 0] <= thr).any()), bool((d[:, 1] <= thr).any())
            c0, c1 = int(tree.child[cur, 0]), int(tree.child[cur, 1])
            if v0 and v1:
                first0 = d[center, 0] <= d[center, 1]
                stack.append(c1 if first0 else c0)
                cur = c0 if first0 else c1
            elif v0:
                cur = c0
            elif v1:
                cur = c1
            else:
                if not stack:
                    break
                cur = stack.pop()
    return st


def lattice_packet(res, bx, by, bz):
    """the 64 points of the 4^3 block (bx, by, bz) of the res^3 lattice over [-1, 1]^3; lanes beyond the lattice are parked on a
    clamped copy, as the kernel does"""
    l = np.arange(64)
    ix, iy, iz = 4 * bx + (l & 3), 4 * by + ((l >> 2) & 3), 4 * bz + (l >> 4)
    live = (ix < res) & (iy < res) & (iz < res)
    idx = np.stack([np.minimum(ix, res - 1), np.minimum(iy, res - 1), np.minimum(iz, res - 1)], 1)
    return idx / (res - 1) * 2.0 - 1.0, live


def model(tree, res, packets=400, seed=0):
    nb = (res + 3) // 4
    if packets and packets < nb ** 3:
        rs = np.random.RandomState(seed)
        blocks = rs.randint(0, nb, (packets, 3))
    else:
        g = np.arange(nb)
        blocks = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tot = None
    for bx, by, bz in blocks:
        P, live = lattice_packet(res, int(bx), int(by), int(bz))
        st = walk(tree, P, live)
        tot = st if tot is None else {k: tot[k] + st[k] for k in st}
    n = len(blocks)
    out = {k: v / n for k, v in tot.items()}
    out["packets"] = n
    return out


def mesh_by_name(name):
    from icon_amd import synth
    a = synth.make_assets(name)
    return np.asarray(a.smpl_verts[0], np.float32), np.asarray(a.smpl_faces[0], np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", default="body")
    ap.add_argument("--res", type=int, default=257)
    ap.add_argument("--packets", type=int, default=400, help="random 4^3 packets of the lattice (0: all of them)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    v, f = mesh_by_name(a.mesh)
    r = model(Tree(v, f), a.res, a.packets, a.seed)
    print(f"mesh {a.mesh}, {a.res}^3 lattice, {r['packets']} packets (seed {a.seed}); per 4^3 packet (mean):")
    print(f"  nodes visited                                   {r['nodes']:8.1f}")
    print(f"  leaves visited                                  {r['leaves']:8.1f}")
    print(f"  triangle tests / within reach of some lane      {r['tris']:8.1f} / {r['tris_useful']:.1f}")
    print(f"  visited leaves with no triangle within reach    {100 * r['leaves_useless'] / max(r['leaves'], 1e-9):8.1f} %")
    print(f"  leaf pairs offered to the distance test         {r['offered']:8.1f}")
    print(f"  pairs with a useful triangle (ceiling)          {r['useful']:8.1f}")
    print(f"  pairs surviving the oriented box                {r['boxed']:8.1f}  ({100 * r['boxed'] / max(r['offered'], 1e-9):.0f} %)")
    print(f"  visited leaves with both pairs culled           {100 * r['leaves_boxed_out'] / max(r['leaves'], 1e-9):8.1f} %")


if __name__ == "__main__":
    main()

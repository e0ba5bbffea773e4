"""The node boxes (mesh_rules.h: range_box_setup / node_box_make; common.h: BvhNode::nb_child) on the host, through the host
builder's arena (icon_debug_host_mesh_build): (a) exactly the parents whose children both hold at most kNodeBoxMaxTris triangles
carry a record, with an orthonormal (or the identity) frame and the flagged child references; (b) the float32 bound the walk
evaluates (icon_debug_box_bound: pair_box_bound itself) never exceeds the float64 squared distance to the nearest triangle of the
child's slot range - no tolerance, no exceptions; (c) a float64 restatement of the whole walk (tools/node_box_model.py) returns
the same 64 keys per packet with the boxes as without, for every packet of the 33^3 lattice."""
import numpy as np
import pytest

from node_box_cases import K_FLAG, K_MAX_TRIS, STRIPS, box_bound, mesh, model, range_box

MESHES = ["body", "ico", "tiny", "dup", "line"] + list(STRIPS)
pbm = model.pbm


@pytest.fixture(scope="module")
def points():
    g = np.linspace(-1.0, 1.0, 33)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    return lattice, cube


_trees = {}


def tree_of(name):
    if name not in _trees:
        v, f, _, _ = mesh(name)
        _trees[name] = model.NodeTree(v, f)
    return _trees[name]


def child_ranges(tree, op):
    """every child of every oriented parent: (node [R], side [R], begin [R], end [R])"""
    ids = np.nonzero(op)[0]
    node = np.repeat(ids, 2); side = np.tile([0, 1], len(ids))
    begin = np.where(side == 0, tree.begin[node], node + 1)
    end = np.where(side == 0, node + 1, tree.end[node])
    return node, side, begin, end


@pytest.mark.parametrize("name", MESHES)
def test_records_sit_on_exactly_the_oriented_parents(name):
    tree = tree_of(name)
    F = tree.F
    op = tree.oriented(K_MAX_TRIS)
    has, _ = tree.arena_boxes()
    assert np.array_equal(op, has)
    assert not tree.nbox[~op].any()                                       # nothing else is written
    if name in ("strip1", "strip2", "tiny"):
        assert tree.root < 0 and not op.any()                             # the root is a leaf
    if name in ("strip16", "strip17"):
        assert tree.root >= 0 and op[tree.root]                           # the root is an oriented parent (of 16 / of more than 16 triangles)
    if name == "strip33":
        assert tree.root >= 0 and not op[tree.root] and op.any()          # a child of the root is over the threshold (33 = 16 + 17 at best)
    if name == "body":
        assert (int(op.sum()), int(tree.is_node.sum())) == (3828, 4500)
    # the references the walk follows: the plain ones, an inner child that is an oriented parent flagged
    nodes = np.nonzero(tree.is_node)[0]
    ch = tree.child[nodes].astype(np.int64)
    flagged = np.where((ch >= 0) & op[np.clip(ch, 0, F - 1)], ch | K_FLAG, ch)
    assert np.array_equal(tree.walk_child[nodes], flagged)
    assert np.array_equal(tree.nbox[op][:, 15].view(np.int32), tree.walk_child[op])
    inner = ch[op[nodes]]
    assert ((inner < 0) | op[np.clip(inner, 0, F - 1)]).all()             # an inner child of an oriented parent is one itself
    # frames: orthonormal to 1e-5 (stored times kPairBoxScale), or the identity
    node, side, begin, end = child_ranges(tree, op)
    assert ((end - begin >= 1) & (end - begin <= K_MAX_TRIS)).all()
    ax = tree.nbox[node, 3:12, side].astype(np.float64).reshape(-1, 3, 3) / np.float64(np.float32(0.9999))
    gram = np.einsum("rak,rbk->rab", ax, ax) - np.eye(3)
    ident = (np.abs(ax - np.eye(3)) < 1e-6).all((1, 2))
    assert ((np.abs(gram) <= 1e-5).all((1, 2)) | ident).all()
    assert np.isfinite(tree.nbox[op][:, :15]).all() and (tree.nbox[op][:, 12:15] > 0).all()
    if name == "body":
        assert (~ident).mean() > 0.95                                     # on a surface mesh the oriented frame is the rule
    # ... and the arena holds the rule's own records (spot check through the rule's host entry)
    for k in range(0, len(node), max(1, len(node) // 40)):
        rec, kind = range_box(tree.tri[begin[k]:end[k]])
        assert kind in (0, 1) and np.array_equal(rec.view(np.uint32), tree.nbox[node[k], :15, side[k]].view(np.uint32))


def range_d2(tris, pts):
    """float64 min over a range's triangles; tris [R,K,3,3] (short ranges repeat their last triangle), pts [R,N,3] -> [R,N]"""
    t = tris.astype(np.float64); p = pts.astype(np.float64)
    out = np.full(p.shape[:2], np.inf)
    for k in range(t.shape[1]):
        out = np.minimum(out, pbm.tri_dist2(p, t[:, None, k]))
    return out


@pytest.mark.parametrize("name", MESHES)
def test_bound_never_exceeds_the_float64_distance(name, points):
    lattice, cube = points
    tree = tree_of(name)
    op = tree.oriented(K_MAX_TRIS)
    node, side, begin, end = child_ranges(tree, op)
    R = len(node)
    if R == 0:
        return                                                             # (the root is a leaf: no record, checked above)
    slots = np.minimum(begin[:, None] + np.arange(K_MAX_TRIS)[None], end[:, None] - 1)
    tris = tree.tri[slots]                                                 # [R, 16, 3, 3]
    # on and within 1e-4 of the surface: three points at each of 12 corners / edge midpoints spread over the range (one ON it)
    rs = np.random.RandomState(11)
    c = tris.astype(np.float64).reshape(R, 48, 3)
    base = np.concatenate([c[:, ::8], 0.5 * (c[:, 0:48:9] + c[:, 1:48:9])], 1)       # [R, 12, 3]: corner 0 / edge ab of every third triangle
    off = rs.uniform(-1.0, 1.0, (R, 12, 3, 3)) * (1e-4 / np.sqrt(3.0))
    off[:, :, 0] = 0.0
    near = (base[:, :, None, :] + off).reshape(R, 36, 3).astype(np.float32)
    nl = max(32, -(-100000 // R), -(-len(lattice) // R))                   # >= 100,000 points per mesh, every lattice point used
    il = (np.arange(R)[:, None] * nl + np.arange(nl)[None]) % len(lattice)
    assert R * (nl + 44) >= 100000 and (nl >= len(lattice) or len(np.unique(il)) == len(lattice))
    pts = np.concatenate([lattice[il], np.broadcast_to(cube[None], (R, 8, 3)), near], 1)
    N = pts.shape[1]
    # the bound as the kernel evaluates it: the arena's records, both packed components, float32
    ids = np.nonzero(op)[0]
    bound = box_bound(tree.nbox[ids], pts.reshape(len(ids), 2 * N, 3), False)        # [ids, 2, 2N]: both children at both point sets
    bd = np.stack([bound[:, 0, :N], bound[:, 1, N:]], 1).reshape(R, N).astype(np.float64)
    assert not np.isnan(bd).any()
    for a in range(0, R, 256):
        b = min(R, a + 256)
        d2 = range_d2(tris[a:b], pts[a:b])
        bad = bd[a:b] > d2
        assert not bad.any(), (f"bound above the float64 squared distance (mesh, node, child, point, bound, d2): "
                               f"{(name, int(node[a + np.argwhere(bad)[0][0]]), int(side[a + np.argwhere(bad)[0][0]]), int(np.argwhere(bad)[0][1]), float(bd[a:b][bad][0]), float(d2[bad][0]))}")
    # a point ON the range is never pruned
    assert (bd[:, nl + 8::3] == 0).all()


def test_degenerate_and_non_finite_ranges():
    a, b, c = np.array([0.1, -0.2, 0.3]), np.array([0.4, 0.1, -0.2]), np.array([-0.3, 0.5, 0.1])
    tri = np.stack([a, b, c]).astype(np.float32)
    ident = np.float32(0.9999) * np.eye(3, dtype=np.float32).reshape(-1)
    v, f, _, _ = mesh("tiny")
    closed = v[f]                                                          # a closed surface: the area normals sum to zero
    for name, t in {"closed": closed, "opposed": np.stack([tri, tri[[0, 2, 1]]]), "point": np.stack([np.stack([a] * 3)] * 5).astype(np.float32)}.items():
        rec, kind = range_box(t)
        assert kind == 1 and np.array_equal(rec[3:12], ident), (name, kind, rec)       # the identity frame: the AABB
        lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
        assert np.allclose(rec[:3], 0.5 * (lo + hi), atol=1e-6) and (rec[12:15] >= np.float32(0.9999) * 0.5 * (hi - lo)).all()
    for val in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0, 0), (6, 2, 1), (15, 1, 2)):
            t = np.stack([tri + 0.01 * k for k in range(16)]).astype(np.float32)
            t[pos] = val
            rec, kind = range_box(t)
            assert kind == 2 and np.isinf(rec[12:15]).all()
            recs = np.zeros((1, 16, 2), np.float32); recs[0, :15, 0] = rec; recs[0, :15, 1] = rec
            assert (box_bound(recs, np.float32([[0.9, 0.9, 0.9], [-1, 1, -1], [np.nan, 0, 0]]), True) == 0).all()
    # one triangle: the pair-box rule of a pair that holds it twice
    from pair_box_cases import pair_box
    r1, k1 = range_box(tri[None])
    r2, k2, _ = pair_box(np.concatenate([tri, tri])[None], np.zeros((1, 3), np.float32), True)
    assert k1 == k2[0] == 0 and np.array_equal(r1.view(np.uint32), r2[0].view(np.uint32))


@pytest.mark.parametrize("name", ["body", "ico"])
def test_float64_walk_finds_the_same_keys(name):
    """every packet of the 33^3 lattice (the last ones are one point wide): model() asserts the 64 keys of every packet"""
    tree = tree_of(name)
    blocks = model.blocks_of(33, 0, 0)
    assert len(blocks) == 9 ** 3
    r = model.model(tree, 33, blocks, {"off": None, "on": tree.arena_boxes()})
    print(f"\n{name} 33^3, per packet: off {r['off']}\n                     on  {r['on']}")
    assert r["on"]["obox"] > 0 and r["off"]["obox"] == 0
    # the lockstep walk without node boxes is pair_box_model's one-packet walk (other code, the same definition), count for count
    sub = blocks[::61]
    pk = [pbm.lattice_packet(33, int(x), int(y), int(z)) for x, y, z in sub]
    st, _, _ = model.walk_many(tree, np.stack([p for p, _ in pk]), np.stack([l for _, l in pk]), None)
    one = [pbm.walk(tree, p, l) for p, l in pk]
    assert (st["aabb"], st["leaves"], st["offered"], st["tested"]) == tuple(sum(o[k] for o in one) for k in ("nodes", "leaves", "offered", "boxed"))
    assert r["on"]["aabb"] + r["on"]["obox"] + r["on"]["leaves"] < r["off"]["aabb"] + r["off"]["leaves"]

"""The oriented boxes of the leaf pairs (common.h: PairBox; mesh_rules.h: pair_box_setup / pair_box_bound) on the host: the packet
walk skips a leaf pair when the box's float32 bound exceeds every lane's pruning threshold, so the bound must NEVER exceed the
real squared distance from the point to the pair's triangles - checked here with no tolerance against a float64 distance, through
icon_debug_pair_box, which is compiled from the very function the kernel evaluates (both packed components are exercised).

Every leaf pair of the project's own tree (read from the host builder's arena) of five meshes, four kinds of points:
the 33^3 lattice, 10^4 random points of the cube, points within 1e-4 of corners and edge midpoints, the cube's corners.  The
tetrahedron takes every point for every pair; on the large ones every pair takes the cube's corners, the near points of ITS OWN
corners and edges (where the bound is tightest) and of another pair's, and a slice of the lattice and of the random points that
rotates through all of them over the pairs - 2 to 6 million (pair, point) checks per mesh instead of 300 million."""
import numpy as np
import pytest

from pair_box_cases import mesh, model, pair_box

N_LATTICE, N_RANDOM = 192, 96          # per pair at least, on the large meshes


@pytest.fixture(scope="module")
def points():
    g = np.linspace(-1.0, 1.0, 33)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rs = np.random.RandomState(5)
    random = rs.uniform(-1.0, 1.0, (10000, 3)).astype(np.float32)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    return lattice, random, corners


def near_points(corners, rs):
    """[P, 36, 3]: three points within 1e-4 of each of the pair's six corners and six edge midpoints (one of them ON it)"""
    c = corners.astype(np.float64)
    mids = np.stack([0.5 * (c[:, i] + c[:, j]) for i, j in ((0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5))], 1)
    base = np.concatenate([c, mids], 1)                                   # [P, 12, 3]
    off = rs.uniform(-1.0, 1.0, (len(c), 12, 3, 3)) * (1e-4 / np.sqrt(3.0))
    off[:, :, 0] = 0.0
    return (base[:, :, None, :] + off).reshape(len(c), 36, 3).astype(np.float32)


def pair_d2(corners, pts):
    """float64 min over the pair's two triangles; corners [P,6,3], pts [P,N,3] -> [P,N]"""
    tri = corners.astype(np.float64).reshape(len(corners), 2, 3, 3)
    p = pts.astype(np.float64)
    return np.minimum(model.tri_dist2(p, tri[:, None, 0]), model.tri_dist2(p, tri[:, None, 1]))


def check(corners, pts, shared, what):
    rec, kind, bound = pair_box(corners, pts, shared)
    P = len(corners)
    worst = None
    for a in range(0, P, 512):                                             # chunks keep the float64 temporaries small
        b = min(P, a + 512)
        pp = np.broadcast_to(pts[None], (b - a,) + pts.shape) if shared else pts[a:b]
        d2 = pair_d2(corners[a:b], pp)
        bd = bound[a:b].astype(np.float64)
        assert not np.isnan(bd).any(), what
        bad = bd > d2
        if bad.any():
            i, j = np.argwhere(bad)[0]
            worst = (what, int(a + i), int(j), float(bd[i, j]), float(d2[i, j]), int(kind[a + i]))
            break
    assert worst is None, f"bound above the float64 squared distance (mesh, pair, point, bound, d2, kind): {worst}"
    return rec, kind, bound


@pytest.mark.parametrize("name", ["body", "ico", "line", "dup", "tiny"])
def test_bound_never_exceeds_the_float64_distance(name, points):
    lattice, random, cube = points
    v, f, _, _ = mesh(name)
    tree = model.Tree(v, f)
    leaf, pr, s0, s1 = tree.pairs()
    corners = np.concatenate([tree.tri[s0], tree.tri[s1]], 1)             # [P, 6, 3]
    P = len(corners)
    assert P >= 1 and set(np.concatenate([s0, s1]).tolist()) == set(range(len(f)))       # every triangle is in a pair
    rs = np.random.RandomState(11)
    near = near_points(corners, rs)
    if P <= 16:                                                             # every pair x every point
        shared = np.concatenate([lattice, random, cube, near.reshape(-1, 3)])
        rec, kind, _ = check(corners, shared, True, name)
    else:
        nl, nr = max(N_LATTICE, -(-len(lattice) // P)), max(N_RANDOM, -(-len(random) // P))      # (enough to use all of both)
        il = (np.arange(P)[:, None] * nl + np.arange(nl)[None]) % len(lattice)
        ir = (np.arange(P)[:, None] * nr + np.arange(nr)[None]) % len(random)
        assert len(np.unique(il)) == len(lattice) and len(np.unique(ir)) == len(random)       # all of both are used
        pts = np.concatenate([lattice[il], random[ir], np.broadcast_to(cube[None], (P, 8, 3)), near, near[rs.permutation(P)]], 1)
        rec, kind, _ = check(corners, pts, False, name)
    # the arena of the host builder holds exactly these records (short leaves repeat their last pair's box; field 15 is 0)
    assert np.array_equal(tree.pbox[leaf, :15, pr].view(np.uint32), rec.view(np.uint32))
    assert not tree.pbox[:, 15].any()
    short = np.nonzero((tree.leaf_cnt > 0) & (tree.leaf_cnt <= 2))[0]
    assert np.array_equal(tree.pbox[short, :, 0].view(np.uint32), tree.pbox[short, :, 1].view(np.uint32))
    assert (kind != 2).all()                                               # finite meshes: every pair has a real box
    if name in ("body", "ico"):
        assert (kind == 0).mean() > 0.95                                   # ... and on a surface mesh it is the oriented one


def test_degenerate_and_non_finite_pairs_never_cull_wrongly(points):
    lattice, random, cube = points
    rs = np.random.RandomState(3)
    a, b, c = np.array([0.1, -0.2, 0.3]), np.array([0.4, 0.1, -0.2]), np.array([-0.3, 0.5, 0.1])
    tri = np.stack([a, b, c])
    deg = {
        "point": np.stack([a] * 6),                                        # zero area, zero length
        "collinear": np.stack([a, b, a + 0.25 * (b - a), a, b, a + 0.75 * (b - a)]),
        "sliver": np.stack([a, b, a + 0.5 * (b - a) + 1e-9, a, b, a + 0.3 * (b - a) - 1e-9]),
        "opposed": np.concatenate([tri, tri[[0, 2, 1]]]),                   # the two normals cancel
        "zero+tri": np.concatenate([np.stack([b] * 3), tri]),
    }
    corners = np.stack(list(deg.values())).astype(np.float32)
    pts = np.concatenate([lattice[::7], random[:2000], cube, near_points(corners, rs).reshape(-1, 3)])
    rec, kind, bound = check(corners, pts, True, "degenerate")
    ident = np.float32(0.9999) * np.eye(3, dtype=np.float32).reshape(-1)
    for k, name in enumerate(deg):
        if name != "zero+tri":                                             # (one good triangle is enough for a frame)
            assert kind[k] == 1 and np.array_equal(rec[k, 3:12], ident), (name, kind[k], rec[k])
    # a degenerate pair's AABB still prunes what is far from it - and a point ON the pair is never pruned
    assert (bound[:, -36 * len(deg):] .reshape(len(deg), len(deg), 36)[np.arange(len(deg)), np.arange(len(deg)), ::3] == 0).all()
    # non-finite corners: infinite extents, the bound is 0 for every point
    bad = []
    for val in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0), (2, 1), (4, 2), (5, 0)):
            t = np.concatenate([tri, tri + 0.05]).astype(np.float32)
            t[pos] = val
            bad.append(t)
    bad.append(np.concatenate([tri, tri * 3e38]).astype(np.float32))       # finite corners whose box overflows float32
    bad = np.stack(bad)
    far = np.concatenate([cube, random[:500], np.float32([[1e18, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1]])])
    rec, kind, bound = pair_box(bad, far, True)
    assert (kind[:-1] == 2).all() and np.isinf(rec[:-1, 12:15]).all() and (bound[:-1] == 0).all()
    assert kind[-1] in (1, 2) and not np.isnan(bound[-1, :-2]).any()
    # NaN points are never pruned either (the bound is 0, never NaN), whatever the box
    good = np.concatenate([tri, tri + 0.05])[None].astype(np.float32)
    _, _, bn = pair_box(good, np.float32([[np.nan, 0, 0], [0, np.nan, 0], [np.nan] * 3]), True)
    assert (bn == 0).all()

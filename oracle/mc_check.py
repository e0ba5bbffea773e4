"""Independent checker of the marching-cubes output - TEST INFRASTRUCTURE ONLY.

The reference extracts the mesh with third-party code that is absent here (kaolin
``voxelgrids_to_trianglemeshes`` for grids <= 256^3, PyMCubes above: lib/common/seg3d_lossless.py:583-604),
so there is no reference output to compare triangle lists with: PARITY UNPINNED for the triangulation.
What every correct marching cubes shares, whatever its case table, is checked here in plain numpy, written
without looking at the product's tables:

* the VERTEX SET: one vertex on every lattice edge whose end points lie on different sides of the level
  (``a > level`` xor ``b > level``), at the linear interpolation ``i + (level - a) / (b - a)``;
* every triangle joins three crossings of ONE cube;
* the surface is a closed, consistently oriented 2-manifold (every directed edge has exactly one
  opposite partner) wherever it does not touch the border of the grid, with the inside (occ > level)
  on the side the reference's conventions put it (positive signed volume after export_mesh's
  ``faces[:, [0, 2, 1]]`` flip means outward normals);
* Euler characteristic 2 per closed genus-0 component (reported, asserted by the caller where the
  topology is known).

export_mesh conventions (seg3d_lossless.py:585-602): marching cubes on ``occ[1:, 1:, 1:]``, vertices as
(x, y, z) in voxel units of the cropped grid.
"""
from __future__ import annotations

import numpy as np


def edge_crossings(occ: np.ndarray, level: float = 0.5) -> np.ndarray:
    """[N,3] float64 (x, y, z) positions of all level crossings on the lattice edges of ``occ[1:,1:,1:]``
    (z slowest in the array, as the reference's volume)."""
    v = np.asarray(occ, np.float32)[1:, 1:, 1:]
    ins = v > np.float32(level)
    out = []
    for axis in (0, 1, 2):                         # array axes: 0 = z, 1 = y, 2 = x
        a = np.moveaxis(v, axis, 0)
        ia = np.moveaxis(ins, axis, 0)
        cross = ia[:-1] != ia[1:]
        idx = np.argwhere(cross)                   # (k along axis, other two in array order)
        va = a[:-1][cross].astype(np.float64)
        vb = a[1:][cross].astype(np.float64)
        t = (np.float64(level) - va) / (vb - va)
        coords = idx.astype(np.float64)
        coords[:, 0] += t
        # back to array order (z, y, x)
        order = [0, 1, 2]
        order.remove(axis)
        zyx = np.empty_like(coords)
        zyx[:, axis] = coords[:, 0]
        zyx[:, order[0]] = coords[:, 1]
        zyx[:, order[1]] = coords[:, 2]
        out.append(zyx[:, ::-1])                   # -> (x, y, z)
    return np.concatenate(out, 0)


def same_point_set(a: np.ndarray, b: np.ndarray, tol: float = 1e-4) -> bool:
    """both [N,3]; equal as (multi)sets up to ``tol``: the same number of points, every point of one has a partner in the other,
    and the matching is one-to-one except among points that COINCIDE within ``tol`` in their own set (a lattice value exactly at
    the level puts the crossings of up to six edges on the lattice point itself - a handful among the 1.4e8 values of a 513^3
    volume - and the nearest-neighbour query may hand all of them the same partner)"""
    from scipy.spatial import cKDTree
    if len(a) != len(b):
        return False
    if len(a) == 0:
        return True
    tb = cKDTree(b)
    da, ia = tb.query(a)
    db, _ = cKDTree(a).query(b)
    if not (da.max() <= tol and db.max() <= tol):
        return False
    twins = tb.query_pairs(tol, output_type="ndarray")
    n_twinned = len(np.unique(twins)) if len(twins) else 0
    return bool(len(np.unique(ia)) >= len(a) - n_twinned)


def topology(verts: np.ndarray, faces: np.ndarray, grid: int) -> dict:
    """``grid`` = points per axis of the cropped volume (vertices lie in [0, grid-1])."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    res = {"n_verts": len(v), "n_faces": len(f)}
    if len(f) == 0:
        res.update(closed=True, oriented=True, euler=0, components=0, signed_volume=0.0, one_cube=True, used_all=len(v) == 0)
        return res
    # every triangle inside one cube
    lo = np.floor(v[f].min(1) + 1e-9)
    hi = v[f].max(1)
    res["one_cube"] = bool((hi <= lo + 1.0 + 1e-6).all())
    res["used_all"] = bool(len(np.unique(f)) == len(v))
    # directed edges
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = e[:, 0] * (len(v) + 1) + e[:, 1]
    rkey = e[:, 1] * (len(v) + 1) + e[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    res["oriented"] = bool((cnt == 1).all())                      # no directed edge twice
    has_partner = np.isin(key, rkey)
    on_border = lambda p: ((p <= 1e-9) | (p >= grid - 1 - 1e-9)).any(-1)
    open_edges = e[~has_partner]
    # an unmatched edge is legitimate only on the border of the grid
    res["closed"] = bool(len(open_edges) == 0 or (on_border(v[open_edges[:, 0]]) & on_border(v[open_edges[:, 1]])).all())
    res["watertight"] = bool(len(open_edges) == 0)
    und = np.unique(np.sort(e, 1), axis=0)
    res["euler"] = int(len(v) - len(und) + len(f))
    # components (union-find over vertices)
    parent = np.arange(len(v))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in und:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(i) for i in np.unique(f)])
    res["components"] = int(len(np.unique(roots)))
    t = v[f]
    res["signed_volume"] = float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)
    return res


def largest_component(verts: np.ndarray, faces: np.ndarray):
    """numpy restatement of lib/dataset/mesh_util.py:778-791 (trimesh split -> most vertices): the component
    with the most referenced vertices (ties: the one containing the lowest-index face); vertices and faces
    keep their relative order.  -> (verts, faces int32)"""
    v = np.asarray(verts)
    f = np.asarray(faces, np.int64)
    parent = np.arange(len(v))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in f:
        for p, q in ((a, b), (a, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    lab = np.array([find(i) for i in range(len(v))])
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    counts = np.bincount(lab[used], minlength=len(v))
    fl = lab[f[:, 0]]
    best = fl[np.nonzero(counts[fl] == counts.max())[0][0]]
    keep_v = (lab == best) & used
    remap = np.cumsum(keep_v) - 1
    return v[keep_v].astype(np.float32), remap[f[fl == best]].astype(np.int32)


def largest_component_by_faces(verts, faces):
    """The rule, as published (trimesh 3.x - the package is absent here; stated from its source, NOT run):
      lib/dataset/mesh_util.py:778-791   mesh_lst = trimesh.Trimesh(verts, faces).split(only_watertight=False)
                                         comp_num = [m.vertices.shape[0] for m in mesh_lst]
                                         mesh_clean = mesh_lst[comp_num.index(max(comp_num))]      -> FIRST of several largest
      trimesh/base.py  Trimesh.split  -> graph.split(self, only_watertight=False)
      trimesh/graph.py split:   adjacency = mesh.face_adjacency;  min_len = 1 (4 only when only_watertight)
                                components = connected_components(edges=adjacency, nodes=arange(len(faces)), min_len=1)
                                return mesh.submesh(components, only_watertight=False)          -> one mesh per component, in order
      trimesh/graph.py face_adjacency: edges sorted per face, grouping.group_rows(edges_sorted, require_count=2) - two faces are
                                adjacent iff they share an edge used by EXACTLY two faces (an edge of 1 or of 3+ faces joins nothing)
      trimesh/graph.py connected_components (scipy engine: csgraph.connected_components labels, grouping.group(labels)): the
                                components come out in order of their label = of the lowest-numbered face each contains; a face
                                without any adjacency is a component of its own (min_len = 1)
      submesh: faces keep their relative order, vertices are the referenced ones in ascending index order, renumbered
    so: most distinct vertices wins, ties go to the component holding the lowest face index - the rule below and icon_clean_mesh's.
    NOT restated (and a difference if it ever matters): Trimesh(verts, faces) is built with process=True, which first MERGES
    vertices at identical positions (merge_vertices) - marching cubes emits coincident vertices only where a lattice value equals
    the level exactly (a handful per 1.4e8 values, tests/test_gpu_round5.py) - and drops NaN / inf vertices.

    lib/dataset/mesh_util.py:778-791 with trimesh's connectivity spelled out in plain Python (the checker of icon_clean_mesh;
    largest_component above unites faces through shared VERTICES - the two agree except at marching-cubes pinch points):
    faces are adjacent when they share an edge that EXACTLY two faces use (graph.face_adjacency: grouping.group_rows(edges,
    require_count=2)); components of that graph; the one with the most distinct vertices wins (ties: the one holding the
    lowest-index face); vertices and faces keep their order, indices renumbered.  -> (verts float32, faces int32)"""
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    uses = {}
    for i, (a, b, c) in enumerate(f.tolist()):
        for p, q in ((a, b), (b, c), (c, a)):
            uses.setdefault((min(p, q), max(p, q)), []).append(i)
    parent = list(range(len(f)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for fl in uses.values():
        if len(fl) == 2:
            ra, rb = find(fl[0]), find(fl[1])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    lab = np.array([find(i) for i in range(len(f))])
    # distinct vertices per component: the distinct (component, vertex) pairs, counted per component (a loop over the components
    # with a mask each is quadratic on a noise surface, which has thousands of them)
    labs, linv = np.unique(lab, return_inverse=True)
    pairs = np.unique(np.repeat(linv.reshape(-1), 3) * (len(v) + 1) + f.reshape(-1))
    n_verts = np.bincount(pairs // (len(v) + 1), minlength=len(labs))
    best = labs[int(np.argmax(n_verts))] if len(labs) else -1      # ascending, first maximum: of several largest the one with the lowest face
    keep_f = lab == best
    keep_v = np.zeros(len(v), bool)
    keep_v[f[keep_f].reshape(-1)] = True
    remap = np.cumsum(keep_v) - 1
    return v[keep_v], remap[f[keep_f]].astype(np.int32)


def largest_component_scipy(verts, faces):
    """lib/dataset/mesh_util.py:778-791 through the ENGINE trimesh itself calls - scipy.sparse.csgraph.connected_components on
    the face-adjacency graph - with trimesh's own bookkeeping around it restated step by step (trimesh is absent here, scipy is
    not; tests/test_mesh_tools.py pins largest_component_by_faces - the plain-Python checker of icon_clean_mesh - against this):
      geometry.faces_to_edges      edges = faces[:, [0,1,1,2,2,0]].reshape(-1, 2), edge k belongs to face k // 3
      graph.face_adjacency         edges sorted per row; grouping.group_rows(edges_sorted, require_count=2): rows that occur
                                   EXACTLY twice; adjacency = the two faces of each such row (a face adjacent to itself dropped)
      graph.connected_components   engine 'scipy': coo_matrix over the F faces, csgraph.connected_components(directed=False)
                                   -> labels; grouping.group(labels, min_len=1): order = labels.argsort(); one group per label
                                   value in ascending label order - scipy numbers components in order of their lowest node, so
                                   components come out ordered by the lowest face index each holds.  Inside a group the faces
                                   are in ARGSORT order: numpy's default sort is not stable, so the face order inside a
                                   submesh is whatever that sort leaves (ascending whenever it happens to be stable)
      Trimesh.submesh / util.submesh   vertices = the referenced ones in ascending index order (np.unique), faces renumbered
                                   in the group's order
      clean_mesh                   comp_num = vertices per component; index(max) = the FIRST of several largest
    -> (verts float32, faces int32, faces_in_ascending_order: bool)"""
    from scipy.sparse import coo_matrix, csgraph
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    edges = f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)
    edges_face = np.repeat(np.arange(F), 3)
    es = np.sort(edges, axis=1)
    key = es[:, 0] * (int(f.max()) + 1) + es[:, 1]                 # grouping.hashable_rows packs integer rows into one int64 like this
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    length = np.diff(np.concatenate([start, [len(ks)]]))
    two = start[length == 2]
    adj = np.stack([edges_face[order[two]], edges_face[order[two + 1]]], 1)
    adj = adj[adj[:, 0] != adj[:, 1]]
    graph = coo_matrix((np.ones(len(adj), dtype=bool), (adj[:, 0], adj[:, 1])), dtype=bool, shape=(F, F))
    _, labels = csgraph.connected_components(graph, directed=False)
    lorder = labels.argsort()                                      # grouping.group: default kind, as trimesh calls it
    ls = labels[lorder]
    gstart = np.flatnonzero(np.concatenate([[True], ls[1:] != ls[:-1]]))
    glen = np.diff(np.concatenate([gstart, [len(ls)]]))
    groups = [lorder[a:a + n] for a, n in zip(gstart, glen)]
    comp_num = [len(np.unique(f[g].reshape(-1))) for g in groups]
    g = groups[comp_num.index(max(comp_num))]
    used = np.unique(f[g].reshape(-1))
    remap = np.zeros(len(v), np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f[g]].astype(np.int32), bool(np.all(np.diff(g) > 0))

"""The cloth refinement step (icon_amd/cloth.py) stated independently in plain torch with autograd - index_select,
cross, det, cosine_similarity - from the definitions: pytorch3d's published mesh_edge_loss / mesh_normal_consistency /
mesh_laplacian_smoothing(method="uniform") and the mathematics of LocalAffine.  float64 is the reference; the same statement in
float32 on the CPU gives the gaps the GPU bars are taken from (tests/test_cloth.py::test_gaps_are_the_recorded_ones).

The topology is built here by brute force in numpy (python dictionaries), NOT by icon_amd.cloth.ClothTopology, which
tests/test_cloth.py checks against it."""
import itertools

import numpy as np
import torch

from icon_amd import synth

W_CLOTH, W_STIFF, W_RIGID, W_LAP, W_EDGE, W_NC = 10.0, 1e5, 1e5, 1e2, 1.0, 1.0   # the chain's weights (infer.py's, edge and nc at 1)
COS_EPS = 1e-8


# ---- topology, brute force ---------------------------------------------------------------------------------------------------
def topology_np(faces, V):
    """-> dict: edges [E,2] (unique (min, max), ascending min V + max), nbr rows (list of V sorted lists, multiplicity kept),
    pairs [P,4] = (v0, v1, a, c) edge by edge, within an edge the combinations of the corners' positions 3 f + k in order"""
    faces = np.asarray(faces, np.int64)
    corners = {}                                                           # (min, max) -> [(position, third vertex)]
    for fi, f in enumerate(faces):
        for k in range(3):
            a, b = int(f[(k + 1) % 3]), int(f[(k + 2) % 3])
            corners.setdefault((min(a, b), max(a, b)), []).append((3 * fi + k, int(f[k])))
    keys = sorted(corners, key=lambda e: e[0] * V + e[1])
    edges = np.array(keys, np.int64).reshape(-1, 2)
    rows = [[] for _ in range(V)]
    for a, b in keys:
        rows[a].append(b)
        rows[b].append(a)
    rows = [sorted(r) for r in rows]
    pairs = []
    for e in keys:
        lst = sorted(corners[e])
        for (_, a), (_, c) in itertools.combinations(lst, 2):
            pairs.append((e[0], e[1], a, c))
    return {"edges": edges, "rows": rows, "pairs": np.array(pairs, np.int64).reshape(-1, 4)}


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def local_affine(x, A, b, edges):
    """x [B,V,3], A [B,V,3,3], b [B,V,3,1], edges [E,2] long -> y [B,V,3], stiffness mean, rigidity mean"""
    y = (torch.matmul(A, x.unsqueeze(3)) + b).squeeze(3)
    w = torch.cat((A, b), dim=3)
    diff = torch.index_select(w, 1, edges[:, 0]) - torch.index_select(w, 1, edges[:, 1])
    return y, (diff ** 2).mean(), ((torch.linalg.det(A) - 1.0) ** 2).mean()


def edge_loss(y, edges, target_length=0.0):
    if edges.shape[0] == 0:
        return y.sum() * 0.0
    d = torch.index_select(y, 0, edges[:, 0]) - torch.index_select(y, 0, edges[:, 1])
    return ((d.norm(dim=1, p=2) - target_length) ** 2).sum() / edges.shape[0]


def laplacian_loss(y, edges):
    V = y.shape[0]
    s = torch.zeros_like(y).index_add(0, edges[:, 0], torch.index_select(y, 0, edges[:, 1]))
    s = s.index_add(0, edges[:, 1], torch.index_select(y, 0, edges[:, 0]))
    deg = (torch.bincount(edges[:, 0], minlength=V) + torch.bincount(edges[:, 1], minlength=V)).to(y.dtype)
    r = s / deg.clamp(min=1.0).unsqueeze(1) - y
    return r.norm(dim=1, p=2).sum() / V


def normal_consistency(y, pairs):
    if pairs.shape[0] == 0:
        return y.sum() * 0.0
    v0, v1, a, c = (torch.index_select(y, 0, pairs[:, k]) for k in range(4))
    n0 = torch.cross(v1 - v0, a - v0, dim=1)
    n1 = -torch.cross(v1 - v0, c - v0, dim=1)
    return (1.0 - torch.cosine_similarity(n0, n1, dim=1, eps=COS_EPS)).sum() / pairs.shape[0]


def priors(y, edges, pairs, target_length=0.0):
    return edge_loss(y, edges, target_length), normal_consistency(y, pairs), laplacian_loss(y, edges)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def ico():
    """icosahedron subdivided twice: V = 162, F = 320, closed manifold"""
    v, f = synth.icosphere(2)
    return v.astype(np.float32), f.astype(np.int64)


def _sheet(nx, ny):
    """nx x ny vertices at integer (i, j, 0), vertex j nx + i; every cell split along (i, j) - (i + 1, j + 1)"""
    v = np.array([[i, j, 0] for j in range(ny) for i in range(nx)], np.float32)
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            f += [(a, b, d), (a, d, c)]
    return v, np.array(f, np.int64)


def flat():
    """the 9 x 7 sheet on integer coordinates: every interior residual of the uniform Laplacian is exactly 0 in any precision
    (six neighbours at offsets that cancel, a sum of small integers divided by 6), every pair of faces exactly coplanar"""
    return _sheet(9, 7)


def grid():
    """the same sheet, scaled to 0.1 and jittered in all three coordinates: boundary edges, so P < E"""
    v, f = _sheet(9, 7)
    rs = np.random.RandomState(97)
    return (v * 0.1 + rs.normal(scale=0.02, size=v.shape)).astype(np.float32), f


def fan():
    """non-manifold: vertex 0 is the hub of a closed fan over the ring 1..40 (degree 40); three faces share the edge (41, 42) -
    3 pairs; vertex 46 belongs to no face"""
    rs = np.random.RandomState(41)
    ang = np.arange(40) * (2 * np.pi / 40)
    ring = np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.05 * rs.normal(size=40)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.2]], ring,
                        [[0.8, -0.2, 0.0], [0.8, 0.2, 0.1], [1.0, 0.0, 0.3], [0.6, 0.05, 0.25], [0.85, 0.0, -0.3]],
                        [[-0.7, 0.7, 0.4]]]).astype(np.float32)
    f = [(0, 1 + k, 1 + (k + 1) % 40) for k in range(40)] + [(41, 42, 43), (42, 41, 44), (41, 42, 45)]
    return v, np.array(f, np.int64)


def v257():
    """a strip of 255 triangles over 257 vertices: one lane per vertex puts the last vertex alone into a second 256-lane workgroup"""
    rs = np.random.RandomState(257)
    k = np.arange(257)
    v = np.stack([0.005 * k - 0.64, 0.01 * (k % 2) + 0.002 * rs.normal(size=257), 0.003 * rs.normal(size=257)], 1).astype(np.float32)
    f = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(255)]
    return v, np.array(f, np.int64)


def body():
    """the committed synthetic body surface: V = 6890, F = 13776, E = 20664 - 81 workgroups of edges: the cross-workgroup reduction.
    (It holds no degenerate face - tests/test_cloth.py asserts it - so its nc gradient is compared like every other.)"""
    v, f = synth.load_body_mesh()
    return v.astype(np.float32), f.astype(np.int64)


def degenerate(scale=1.0):
    """not one of CASES (it takes no part in the gaps): three faces, two pairs, for the clamped branch of the cosine.  Face 0 has
    its third vertex ON its edge (0, 1): zero area, n = 0 exactly on these coordinates in any precision, so the pair over (0, 1)
    has cos = 0 and a gradient of order 1 / eps through the clamped norm; the pair over (0, 3) is an ordinary one.  With
    `scale` = 2^-17 (exact in float32) every cross product is shorter than eps = 1e-8: both norms of both pairs are clamped
    and the n / |n| part of the gradient is live."""
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1]], np.float32) * np.float32(scale)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 3, 4]], np.int64)
    return v, f


CASES = {"ico": ico, "grid": grid, "flat": flat, "fan": fan, "v257": v257, "body": body}
# (case, B, target_length): every case once; ico with two meshes (LocalAffine only: the priors take one); grid with a rest length
RUNS = [(name, 1, 0.0) for name in CASES] + [("ico", 2, 0.0), ("grid", 1, 0.1)]
SCALARS = ("stiffness", "rigid", "edge", "nc", "laplacian")
PRIOR_TERMS = ("edge", "nc", "laplacian")

_mesh_cache, _run_cache = {}, {}


def mesh(name):
    """-> verts [V,3] float32, faces [F,3] int64, topology_np - once per process, never written to"""
    if name not in _mesh_cache:
        v, f = CASES[name]()
        _mesh_cache[name] = (v, f, topology_np(f, len(v)))
    return _mesh_cache[name]


def inputs(name, B=1, seed=0):
    """-> x [B,V,3], A [B,V,3,3] = I + 0.05 N(0,1), b [B,V,3,1] = 0.02 N(0,1), G [B,V,3] = N(0,1): float32 numpy, seeded.  Mesh
    k > 0 of a batch is mesh 0 shrunk and shifted."""
    v = mesh(name)[0]
    rs = np.random.RandomState(1000 * seed + len(v))
    x = np.stack([v * np.float32(1.0 - 0.1 * k) + np.float32(0.01 * k) for k in range(B)]).astype(np.float32)
    A = (np.eye(3)[None, None] + 0.05 * rs.normal(size=(B, len(v), 3, 3))).astype(np.float32)
    b = (0.02 * rs.normal(size=(B, len(v), 3, 1))).astype(np.float32)
    G = rs.normal(size=(B, len(v), 3)).astype(np.float32)
    return x, A, b, G


def run(name, B=1, target_length=0.0, seed=0, dtype=torch.float64):
    """every output the tests compare, as numpy in `dtype`'s precision (cached; never written to):
    LocalAffine on (x, A, b): y, stiffness, rigid and grad_A, grad_b of 10 <y, G> + 1e5 stiffness + 1e5 rigid;
    B = 1 only - the priors on the case's own vertices: edge, nc, laplacian, grad_verts of 1e2 laplacian + edge + nc and
    grad_verts_<term> of each term alone; the chain 10 <y, G> + 1e5 stiffness + 1e5 rigid + 1e2 laplacian(y) + edge(y) + nc(y):
    chain_grad_A, chain_grad_b"""
    key = (name, B, target_length, seed, dtype)
    if key in _run_cache:
        return _run_cache[key]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                # float32 sums in ONE order on every host: the recorded gaps do not depend on the core count
    try:
        _run_cache[key] = _run(name, B, target_length, seed, dtype)
    finally:
        torch.set_num_threads(threads)
    return _run_cache[key]


def _run(name, B, target_length, seed, dtype):
    v, f, topo = mesh(name)
    edges, pairs = torch.from_numpy(topo["edges"]), torch.from_numpy(topo["pairs"])
    x, A, b, G = (torch.from_numpy(t).to(dtype) for t in inputs(name, B, seed))
    out = {}
    A.requires_grad_(True), b.requires_grad_(True)
    y, stiff, rigid = local_affine(x, A, b, edges)
    (W_CLOTH * (y * G).sum() + W_STIFF * stiff + W_RIGID * rigid).backward()
    out.update(y=y, stiffness=stiff, rigid=rigid, grad_A=A.grad, grad_b=b.grad)
    if B == 1:
        verts = torch.from_numpy(v).to(dtype).requires_grad_(True)
        e, n, l = priors(verts, edges, pairs, target_length)
        out.update(edge=e, nc=n, laplacian=l)
        out["grad_verts"], = torch.autograd.grad(W_LAP * l + W_EDGE * e + W_NC * n, verts, retain_graph=True)
        for term, val in zip(PRIOR_TERMS, (e, n, l)):
            out["grad_verts_" + term], = torch.autograd.grad(val, verts, retain_graph=True)
        A2, b2 = A.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        y2, s2, r2 = local_affine(x, A2, b2, edges)
        e2, n2, l2 = priors(y2[0], edges, pairs, target_length)
        (W_CLOTH * (y2 * G).sum() + W_STIFF * s2 + W_RIGID * r2 + W_LAP * l2 + W_EDGE * e2 + W_NC * n2).backward()
        out.update(chain_grad_A=A2.grad, chain_grad_b=b2.grad)
    return {k: t.detach().numpy() for k, t in out.items()}


def rel_scalar(a, ref):
    a, ref = float(a), float(ref)
    if a == ref:
        return 0.0
    return abs(a - ref) / abs(ref) if ref != 0.0 else float("inf")


def rel_grad(g, ref):
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    top = float(np.abs(ref).max())
    d = float(np.abs(g - ref).max())
    return d / top if top > 0.0 else (0.0 if d == 0.0 else float("inf"))


# which recorded gap an output of run() is held to: the chain's gradients share grad_A / grad_b; the weighted sum of the priors is
# dominated by its Laplacian term and shares that term's gap; the edge and nc terms alone have their own, far smaller ones
GAP_OF = {"y": "y", "grad_A": "grad_A", "chain_grad_A": "grad_A", "grad_b": "grad_b", "chain_grad_b": "grad_b",
          "grad_verts": "grad_verts", "grad_verts_laplacian": "grad_verts", "grad_verts_edge": "grad_verts_edge", "grad_verts_nc": "grad_verts_nc"}
GAP_OF.update({s: s for s in SCALARS})


def gap(out, ref, key):
    """how far `out[key]` lies from `ref[key]` in the measure of its kind: scalars relative, y and the gradients
    ||g - ref||inf / ||ref||inf"""
    return rel_scalar(out[key], ref[key]) if key in SCALARS else rel_grad(out[key], ref[key])


def measure_gaps(seeds=range(5)):
    """-> {kind: (largest gap of the float32 oracle against the float64 oracle, (case, B, target_length, seed, output) that set it)}"""
    worst = {}
    for name, B, t in RUNS:
        for seed in seeds:
            r64, r32 = run(name, B, t, seed, torch.float64), run(name, B, t, seed, torch.float32)
            for key in r64:
                g = gap(r32, r64, key)
                kind = GAP_OF[key]
                if kind not in worst or g > worst[kind][0]:
                    worst[kind] = (g, (name, B, t, seed, key))
    return worst

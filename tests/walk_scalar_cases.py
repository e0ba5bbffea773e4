"""What tests/test_gpu_walk_scalar.py compares with tests/golden/walk_scalar_parent.npz and tools/make_golden_walk_scalar.py records:
one function per group of cases, each returning {name: value} with value a SHA-256 of an output's bytes (bit-exact comparison of
arrays too large to commit) or an integer counter.  The library exposes the lattice search's slot words and squared distances only
through what is computed from them - the occupancy volume of eval_slab (every lattice point's nearest slot, d^2 inside the clip band
and sign) - so the volumes stand for them; point queries return face and sdf themselves.
share_waves = 1 makes the small lattices run k_nearest<lattice> itself, the kernel of the 257^3 call."""
import hashlib

import numpy as np
import torch

from common import assets, set_option
from node_box_cases import mesh

DEV = torch.device("cuda:0")
N_POINTS = 100352                                        # just above the packet threshold (98,304): the Morton packet walk
SMALL = ("strip1", "strip2", "strip3", "strip4", "strip5", "strip6", "strip7", "strip8", "tiny")
#         root = a leaf of 1, 2, 3, 4 triangles; strip5 .. strip8: one inner node over two leaves (4 + 1 .. 4 + 4 or an even split); tiny: a closed leaf
SWITCHES = {"both_on": (1, 1), "pair_box_off": (0, 1), "node_box_off": (1, 0), "both_off": (0, 0)}    # (pair_box, node_box), set before the mesh is created


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def digest(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def body_points():
    return np.random.RandomState(7).uniform(-1, 1, (N_POINTS, 3)).astype(np.float32)


def far_points():
    rs = np.random.RandomState(13)
    d = rs.normal(size=(4096, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rs.uniform(5.0, 50.0, (4096, 1))).astype(np.float32)


def lattice_points(res):
    g = np.linspace(-1.0, 1.0, res, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def engine_for(a, mesh_arrays=None, **kw):
    from icon_amd.engine import IconQueryEngine
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, **kw)
    if mesh_arrays is None:
        eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    else:
        v, f, cm, vs = mesh_arrays
        eng.set_mesh(T(v)[None], T(f)[None], T(cm)[None], T(vs)[None])
    eng.set_regressor({k: torch.from_numpy(w) for k, w in a.state_dict.items()})
    return eng


def mesh_handle(name):
    from icon_amd.engine import MeshHandle
    v, f, cm, vs = mesh(name)
    return MeshHandle(T(v), T(f), T(cm), T(vs))


def counters(m, res):
    ws, ps = m.walk_stats(res), m.pair_stats(res)
    out = {k: int(ws[k]) for k in ("packets", "nodes", "oriented_nodes", "leaves", "pairs_offered", "pairs_tested")}
    out.update({"pair_stats_" + k: int(ps[k]) for k in ("packets", "nodes", "pairs_offered", "pairs_tested")})
    return out


def volumes(name, cmap_mode):
    """occupancy volumes at 33^3 (a trimmed tiling that ends in partial packets: parked lanes) and 65^3"""
    a = assets(name)
    eng = engine_for(a, cmap_mode=cmap_mode)
    feat = T(a.features)
    out = {}
    for res in (33, 65):
        vol = eng.eval_slab(feat, res, 0, res)
        assert bool((vol != 0).any())
        out[f"vol/{name}/{cmap_mode}/{res}"] = digest(vol)
    return out


def query_body():
    a = assets("body")
    pts = T(body_points().T.copy())[None]
    occ = engine_for(a).query([T(a.features)], pts, torch.eye(4, device=DEV)[None])[0]
    assert occ.shape[-1] == N_POINTS and bool((occ > 0.5).any()) and bool((occ < 0.5).any())
    return {"query/body": digest(occ)}


def point_queries(name):
    m = mesh_handle(name)
    res = m.sdf_query(T(body_points()))
    m.close()
    if name == "dup":                                    # 3,000 copies of face 0's triangle: wherever one of them wins, it is face 0
        face = res["face"]
        assert bool((face == 0).any()) and not bool(((face > 0) & (face < 3000)).any())
    return {f"points/{name}/{k}": digest(v) for k, v in sorted(res.items())}


def walk_counters(res):
    m = mesh_handle("body")
    out = {f"walk/body/{res}/{k}": v for k, v in counters(m, res).items()}
    m.close()
    return out


def small_mesh(name):
    """a root that is a leaf, one inner node over two leaves, leaves of 1 .. 4 triangles: the 33^3 volume, a point query and the counters"""
    a = assets("body")
    out = {f"small/{name}/vol33": digest(engine_for(a, mesh(name)).eval_slab(T(a.features), 33, 0, 33))}
    m = mesh_handle(name)
    q = m.sdf_query(T(body_points()[:4096]))
    b = m.sdf_query(T(body_points()[:4096]), search="brute")
    for k in ("face", "sdf"):
        assert torch.equal(q[k], b[k]), (name, k)
        out[f"small/{name}/{k}"] = digest(q[k])
    out.update({f"small/{name}/{k}": v for k, v in counters(m, 33).items()})
    m.close()
    return out


def switched(case):
    """the walk with its tables missing: "pair_box" / "node_box" off when the mesh is created"""
    pb, nb = SWITCHES[case]
    set_option("pair_box", pb); set_option("node_box", nb)
    try:
        a = assets("body")
        out = {f"switch/{case}/vol33": digest(engine_for(a).eval_slab(T(a.features), 33, 0, 33))}
        m = mesh_handle("body")
        q = m.sdf_query(T(body_points()))
        for k in ("face", "sdf"):
            out[f"switch/{case}/{k}"] = digest(q[k])
        out.update({f"switch/{case}/{k}": v for k, v in counters(m, 33).items()})
        m.close()
    finally:
        set_option("pair_box", 1); set_option("node_box", 1)
    return out


def far():
    m = mesh_handle("body")
    g, b = m.sdf_query(T(far_points())), m.sdf_query(T(far_points()), search="brute")
    m.close()
    for k in ("face", "sdf"):
        assert torch.equal(g[k], b[k]), k
    return {f"far/{k}": digest(g[k]) for k in ("face", "sdf")}


GROUPS = [(volumes, (n, c)) for n in ("body", "ico") for c in ("reference", "local")] + [(query_body, ())] + \
         [(point_queries, (n,)) for n in ("body", "dup", "line")] + [(walk_counters, (r,)) for r in (33, 65)] + \
         [(small_mesh, (n,)) for n in SMALL] + [(switched, (c,)) for c in SWITCHES] + [(far, ())]


def record_all():
    set_option("share_waves", 1)
    try:
        out = {}
        for fn, args in GROUPS:
            out.update(fn(*args))
        return out
    finally:
        set_option("share_waves", -1)

"""The half-unit, clamped oriented-box bound of the lattice walk (geom_device.h: nearest_packet<.., CLAMP>; mesh_rules.h:
pair_box_bound_half; "box_clamp" option) on the GPU: with the option on, every result is bit for bit what pair_box_bound gives -
volumes, point queries (exact ties included: the lowest face index still wins), the coarse-to-fine schedule - and the walk makes
the SAME visits: the new bound decides what the old one decides wherever the threshold is finite (the body lies inside the cube,
so an excess beyond 2 - the only place the two differ - is met only while the threshold is still infinite).
share_waves = 1 makes the small lattices run k_nearest<lattice> itself (one wavefront per packet), the kernel of the 257^3 call
and the one the option selects; the default launch sizes are run as well.  The option is read when a mesh is created: every case
builds its meshes under the setting it tests."""

import numpy as np
import pytest
import torch

from common import assets, golden, set_option
from node_box_cases import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OCC_TOL = 1e-4                                           # tests/test_gpu_parity.py: the schedule against the reference's own volume


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def options():
    set_option("share_waves", 1)
    yield
    set_option("share_waves", -1)
    set_option("box_clamp", 1)


def make_engine(a, box_clamp, **kw):
    from icon_amd.engine import IconQueryEngine
    set_option("box_clamp", box_clamp)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, **kw)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    eng._mesh_handle()                                   # the mesh is created here, under the option
    return eng


def mesh_handle(name, box_clamp):
    from icon_amd.engine import MeshHandle
    set_option("box_clamp", box_clamp)
    v, f, cm, vs = mesh(name)
    return MeshHandle(T(v), T(f), T(cm), T(vs))


def same_bits(a, b):
    return torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("share_waves", [1, -1])
@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("name", ["body", "ico"])
def test_volumes_are_bit_identical(name, cmap_mode, share_waves):
    set_option("share_waves", share_waves)
    a = assets(name)
    feat = T(a.features)
    out = {}
    for bc in (0, 1):
        eng = make_engine(a, bc, cmap_mode=cmap_mode)
        out[bc] = [eng.eval_slab(feat, res, 0, res).clone() for res in (33, 65)]
    for off, on in zip(out[0], out[1]):
        assert off.shape == on.shape and same_bits(off, on)
    assert any(bool((o != 0).any()) for o in out[1])


def test_query_is_bit_identical():
    """HGPIFuNet.query on 100,352 points (just above the packet threshold, 98,304: the Morton packet walk)"""
    a = assets("body")
    n = 100352
    pts = T(np.random.RandomState(7).uniform(-1, 1, (n, 3)).astype(np.float32).T.copy())[None]
    cal = torch.eye(4, device=DEV)[None]
    occ = {}
    for bc in (0, 1):
        eng = make_engine(a, bc)
        occ[bc] = eng.query([T(a.features)], pts, cal)[0].clone()
    assert occ[0].shape[-1] == n and same_bits(occ[0], occ[1])
    assert bool((occ[1] > 0.5).any()) and bool((occ[1] < 0.5).any())


@pytest.mark.parametrize("name", ["body", "dup", "line"])
def test_point_queries_are_bit_identical(name):
    n = 100352
    pts = T(np.random.RandomState(7).uniform(-1, 1, (n, 3)).astype(np.float32))
    res = {}
    for bc in (0, 1):
        m = mesh_handle(name, bc)
        res[bc] = {k: v.clone() for k, v in m.sdf_query(pts).items()}
        m.close()
    assert set(res[0]) == set(res[1]) and "face" in res[0]
    for k in res[0]:
        assert same_bits(res[0][k], res[1][k]), (name, k)
    if name == "dup":                                    # 3,000 copies of face 0's triangle: wherever one of them wins, it is face 0
        face = res[1]["face"]
        assert bool((face == 0).any()) and not bool(((face > 0) & (face < 3000)).any())


@pytest.mark.parametrize("name", ["dup", "line"])
def test_lattice_on_duplicates_and_slivers(name):
    """the lattice launch (the kernel the option selects) on the 3,000 duplicates and on the slivers: the 33^3 volume, which is a
    function of every lattice point's nearest face and distance, bit for bit"""
    from icon_amd.engine import IconQueryEngine
    a = assets("body")
    v, f, cm, vs = mesh(name)
    out = {}
    for bc in (0, 1):
        set_option("box_clamp", bc)
        eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip)
        eng.set_mesh(T(v)[None], T(f)[None], T(cm)[None], T(vs)[None])
        eng.set_regressor({k: torch.from_numpy(w) for k, w in a.state_dict.items()})
        out[bc] = eng.eval_slab(T(a.features), 33, 0, 33).clone()
    assert same_bits(out[0], out[1])


def test_schedule_is_bit_identical_and_matches_its_golden():
    a = assets("body")
    feat = T(a.features)
    got = {}
    for bc in (0, 1):
        vol, counts, pos = make_engine(a, bc).adaptive_eval(feat, [33, 65, 129, 257])
        got[bc] = (vol.clone(), counts, pos)
    assert same_bits(got[0][0], got[1][0]) and got[0][1:] == got[1][1:]
    g = golden("seg3d_body_adaptive_257.npz")
    assert [int(r) for r in g["resolutions"]] == [33, 65, 129, 257]
    v = got[1][0].reshape(257, 257, 257).cpu().numpy()
    assert np.abs(v[::4, ::4, ::4] - g["sub4"]).max() <= OCC_TOL
    assert np.abs(v[128] - g["plane_z"]).max() <= OCC_TOL and np.abs(v[:, 128] - g["plane_y"]).max() <= OCC_TOL
    assert np.abs(v[:, :, 128] - g["plane_x"]).max() <= OCC_TOL
    assert np.abs(v.reshape(-1)[g["idx"]] - g["samples"]).max() <= OCC_TOL


def test_bvh_search_equals_brute_force_at_33():
    """the lattice's own points, as a point query: the packet walk against the brute-force search, face and sdf bit for bit"""
    g = np.linspace(-1.0, 1.0, 33, dtype=np.float32)
    pts = T(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    m = mesh_handle("body", 1)
    b, w = m.sdf_query(pts, search="brute"), m.sdf_query(pts)
    for k in ("face", "sdf"):
        assert same_bits(w[k], b[k]), k
    m.close()


def test_far_points_equal_brute_force():
    """4,096 points 5 - 50 units outside the cube, where an excess passes 2 and the half-unit bound would stop at its upper limit:
    point mode keeps pair_box_bound for that reason - either setting must serve such points exactly"""
    rs = np.random.RandomState(13)
    d = rs.normal(size=(4096, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = T((d * rs.uniform(5.0, 50.0, (4096, 1))).astype(np.float32))
    for bc in (0, 1):
        m = mesh_handle("body", bc)
        g, b = m.sdf_query(pts), m.sdf_query(pts, search="brute")
        for k in ("face", "sdf"):
            assert same_bits(g[k], b[k]), (bc, k)
        m.close()


@pytest.mark.parametrize("res", [33, 65])
def test_walk_counters_are_exactly_equal(res):
    """AABB visits, oriented visits, leaf visits, pairs offered and pairs tested: the new bound decides what the old one decides"""
    st = {}
    for bc in (0, 1):
        m = mesh_handle("body", bc)
        st[bc] = m.walk_stats(res)
        m.close()
    print(f"\nbox_clamp off: {st[0]}\nbox_clamp on:  {st[1]}")
    assert st[0]["packets"] > 0 and st[1]["oriented_nodes"] > 0 and st[1]["pairs_tested"] < st[1]["pairs_offered"]
    assert st[0] == st[1]

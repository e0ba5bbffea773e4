"""The node boxes of the packet walk (geom_device.h: nearest_packet; "node_box" option) on the GPU: with the oriented boxes on the
bottom inner nodes, every result is bit for bit what the walk on AABBs gives - volumes, point queries (exact ties included: the
lowest face index still wins), the coarse-to-fine schedule - while the walk visits fewer nodes and leaves.  The device builder
writes the same arena as the host builder, the new section included.
share_waves = 1 makes the small lattices run k_nearest<lattice> itself (one wavefront per packet), the kernel of the 257^3 call.
The option is read when a mesh is created: every case builds its meshes under the setting it tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import assets, set_option
from node_box_cases import mesh

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def options():
    set_option("share_waves", 1)
    yield
    set_option("share_waves", -1)
    set_option("node_box", 1)


def make_engine(a, node_box, **kw):
    from icon_amd.engine import IconQueryEngine
    set_option("node_box", node_box)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, **kw)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    eng._mesh_handle()                                   # the mesh is created here, under the option
    return eng


def mesh_handle(name, node_box):
    from icon_amd.engine import MeshHandle
    set_option("node_box", node_box)
    v, f, cm, vs = mesh(name)
    return MeshHandle(T(v), T(f), T(cm), T(vs))


def same_bits(a, b):
    return torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("name", ["body", "ico"])
def test_volumes_are_bit_identical(name, cmap_mode):
    a = assets(name)
    feat = T(a.features)
    out = {}
    for nb in (0, 1):
        eng = make_engine(a, nb, cmap_mode=cmap_mode)
        out[nb] = [eng.eval_slab(feat, res, 0, res).clone() for res in (33, 65)]
    for off, on in zip(out[0], out[1]):
        assert off.shape == on.shape and same_bits(off, on)
    assert any(bool((o != 0).any()) for o in out[1])


@pytest.mark.parametrize("name", ["body", "dup", "line"])
def test_point_queries_are_bit_identical(name):
    n = 100352                                           # just above the packet threshold (98,304): the Morton packet walk
    pts = T(np.random.RandomState(7).uniform(-1, 1, (n, 3)).astype(np.float32))
    res = {}
    for nb in (0, 1):
        m = mesh_handle(name, nb)
        res[nb] = {k: v.clone() for k, v in m.sdf_query(pts).items()}
        m.close()
    assert set(res[0]) == set(res[1]) and "face" in res[0]
    for k in res[0]:
        assert same_bits(res[0][k], res[1][k]), (name, k)
    if name == "dup":                                    # 3,000 copies of face 0's triangle: wherever one of them wins, it is face 0
        face = res[1]["face"]
        assert bool((face == 0).any()) and not bool(((face > 0) & (face < 3000)).any())


def test_schedule_is_bit_identical():
    a = assets("body")
    feat = T(a.features)
    got = {}
    for nb in (0, 1):
        vol, counts, pos = make_engine(a, nb).adaptive_eval(feat, [33, 65, 129, 257])
        got[nb] = (vol.clone(), counts, pos)
    assert same_bits(got[0][0], got[1][0]) and got[0][1:] == got[1][1:]


def test_bvh_search_equals_brute_force():
    pts = T(np.random.RandomState(9).uniform(-1, 1, (4096, 3)).astype(np.float32))
    m = mesh_handle("body", 1)
    g, b = m.sdf_query(pts), m.sdf_query(pts, search="brute")
    for k in ("face", "sdf"):
        assert same_bits(g[k], b[k]), k
    m.close()


@pytest.mark.parametrize("name", ["body", "tiny", "dup", "line", "strip17"])
def test_device_arena_equals_host_arena(name):
    """byte for byte over everything the host builder emits: [dyn's first 80 bytes] and [vnormals, end of the ray-bin lists) - the
    node boxes and the walk references of the nodes included (a zeroed arena: what a build does not write stays 0 in both)"""
    from icon_amd import _lib
    from icon_amd.engine import _stream
    v, f, cm, vs = mesh(name)
    lay = (C.c_int64 * 12)()
    _lib.check(_lib.lib().icon_debug_mesh_layout(C.c_int64(len(v)), C.c_int64(len(f)), lay))
    lay = list(lay)
    host = np.zeros(lay[11], np.uint8)
    _lib.check(_lib.lib().icon_debug_host_mesh_build(_lib.ptr(v), C.c_int64(len(v)), _lib.ptr(f), C.c_int64(len(f)), _lib.ptr(cm), _lib.ptr(vs),
                                                     _lib.ptr(host), C.c_int64(len(host))), "icon_debug_host_mesh_build")
    keep = [T(v), T(f), T(cm), T(vs)]
    arena = torch.zeros(lay[11], dtype=torch.uint8, device=DEV)
    h = C.c_void_p(0)
    _lib.check(_lib.lib().icon_mesh_create_arena(_lib.ptr(keep[0]), C.c_int64(len(v)), _lib.ptr(keep[1]), C.c_int64(len(f)), _lib.ptr(keep[2]),
                                                 _lib.ptr(keep[3]), _lib.ptr(arena), C.c_int64(lay[11]), _stream(), C.byref(h)), "icon_mesh_create_arena")
    try:
        bits = C.c_int(0)
        _lib.check(_lib.lib().icon_mesh_status(h, C.c_int(1), C.byref(bits)), "icon_mesh_status")
        assert bits.value & ~4 == 0, f"status bits {bits.value}"
        dev = arena.cpu().numpy()
        assert np.array_equal(host[lay[0]:lay[0] + 80], dev[lay[0]:lay[0] + 80])
        F = len(f)
        up = lambda n: (n + 255) // 256 * 256
        nb_at = lay[3] + up(384 * F) + up(128 * F)
        for what, a, b in (("nodes", lay[2], lay[3]), ("leaves + pair boxes", lay[3], nb_at), ("node boxes", nb_at, lay[4]), ("the rest", lay[4], lay[10]),
                           ("vnormals", lay[1], lay[2])):
            bad = np.nonzero(host[a:b] != dev[a:b])[0]
            assert len(bad) == 0, f"{name}: {what} differ in {len(bad)} bytes, first at +{bad[0]}"
        if F > 32:
            assert host[nb_at:lay[4]].any()
    finally:
        _lib.lib().icon_mesh_destroy(h)


def test_counters_fewer_visits_no_more_tests():
    """the mechanism at 65^3: strictly fewer node + leaf visits, and the pairs tested stay within 1.1 x the AABB walk's (the model,
    tools/node_box_model.py on every packet of that lattice: 36.1 -> 36.1 per packet)"""
    st = {}
    for nb in (0, 1):
        m = mesh_handle("body", nb)
        st[nb] = m.walk_stats(65)
        m.close()
    print(f"\nnode_box off: {st[0]}\nnode_box on:  {st[1]}")
    assert st[0]["packets"] == st[1]["packets"] > 0
    assert st[0]["oriented_nodes"] == 0 and 0 < st[1]["oriented_nodes"] < st[1]["nodes"]
    assert st[1]["nodes"] + st[1]["leaves"] < st[0]["nodes"] + st[0]["leaves"]
    assert st[1]["pairs_tested"] <= 1.1 * st[0]["pairs_tested"]


def test_the_three_stats_calls_agree():
    """traversal_stats, pair_stats and walk_stats are three launches of one kernel (traversal_stats on pair_box_bound, the other two on
    the walk the mesh runs; the walk is deterministic): the words they share agree exactly - on the
    body (33^3 and 65^3, planes 0..8) and where the root is a leaf (4 triangles) or the only inner node (5 triangles)"""
    for name, res in (("body", 33), ("body", 65), ("strip4", 33), ("strip5", 33)):
        m = mesh_handle(name, 1)
        ts, ps, ws = m.traversal_stats(res, 0, 8), m.pair_stats(res, 0, 8), m.walk_stats(res, 0, 8)
        m.close()
        print(f"\n{name} {res}: {ts}\n  {ps}\n  {ws}")
        assert ts["waves"] == ws["packets"] > 0 and ts["nodes"] == ws["nodes"]
        assert ws["leaves"] <= ts["tris"] <= 4 * ws["leaves"] and ws["leaves"] > 0
        assert [ps[k] for k in ("packets", "nodes", "pairs_offered", "pairs_tested")] == [ws[k] for k in ("packets", "nodes", "pairs_offered", "pairs_tested")]
        # the longest walk is one packet's nodes + triangles: no shorter than the mean, no longer than the sum
        total = ts["nodes"] + ts["tris"]
        assert total <= ts["longest_walk"] * ts["waves"] and ts["longest_walk"] <= total
        if name == "strip4":                                 # the root is a leaf: no inner node, and every packet visits that leaf
            assert ws["nodes"] == 0 and ws["leaves"] == ws["packets"] and ts["tris"] == 4 * ws["packets"] and ts["longest_walk"] == 4
        if name == "strip5":                                 # the root is the only inner node: every packet visits it, and only it
            assert ws["nodes"] == ws["packets"] and ws["leaves"] <= 2 * ws["packets"]

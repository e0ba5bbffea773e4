"""The oriented-box cull of the packet walk (geom_device.h: nearest_packet; "pair_box" option) on the GPU: with the cull on, every
result is bit for bit what the walk without it gives - volumes, point queries (exact ties included: the lowest face index must
still win), the coarse-to-fine schedule - while the walk visits the same nodes and tests strictly fewer leaf pairs.
share_waves = 1 makes the small lattices run k_nearest<lattice> itself (one wavefront per packet), the kernel of the 257^3 call.
The option is read when a mesh is created: every case builds its meshes under the setting it tests."""

import numpy as np
import pytest
import torch

from common import assets, set_option
from pair_box_cases import mesh, model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def options():
    set_option("share_waves", 1)
    yield
    set_option("share_waves", -1)
    set_option("pair_box", 1)


def make_engine(a, pair_box, **kw):
    from icon_amd.engine import IconQueryEngine
    set_option("pair_box", pair_box)
    eng = IconQueryEngine(prior_type="icon", sdf_clip=a.sdf_clip, **kw)
    eng.set_mesh(T(a.smpl_verts), T(a.smpl_faces), T(a.smpl_cmap), T(a.smpl_vis))
    eng.set_regressor({k: torch.from_numpy(v) for k, v in a.state_dict.items()})
    eng._mesh_handle()                                   # the mesh is created here, under the option
    return eng


def mesh_handle(name, pair_box):
    from icon_amd.engine import MeshHandle
    set_option("pair_box", pair_box)
    v, f, cm, vs = mesh(name)
    return MeshHandle(T(v), T(f), T(cm), T(vs))


@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("name", ["body", "ico"])
def test_volumes_are_bit_identical(name, cmap_mode):
    a = assets(name)
    feat = T(a.features)
    out = {}
    for pb in (0, 1):
        eng = make_engine(a, pb, cmap_mode=cmap_mode)
        out[pb] = [eng.eval_slab(feat, res, z0, z1).clone() for res in (33, 65) for z0, z1 in ((0, res), (res // 2 - 2, res // 2 + 5))]
    for off, on in zip(out[0], out[1]):
        assert off.shape == on.shape and torch.equal(off, on)
    assert any(bool((o != 0).any()) for o in out[1])


@pytest.mark.parametrize("name", ["body", "dup", "line"])
def test_point_queries_are_bit_identical(name):
    n = 100352                                           # just above the packet threshold (98,304): the Morton packet walk
    pts = T(np.random.RandomState(7).uniform(-1, 1, (n, 3)).astype(np.float32))
    res = {}
    for pb in (0, 1):
        m = mesh_handle(name, pb)
        res[pb] = {k: v.clone() for k, v in m.sdf_query(pts).items()}
        m.close()
    assert set(res[0]) == set(res[1]) and "face" in res[0]
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        same = torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same, (name, k)


def test_schedule_is_bit_identical():
    a = assets("body")
    feat = T(a.features)
    got = {}
    for pb in (0, 1):
        vol, counts, pos = make_engine(a, pb).adaptive_eval(feat, [33, 65])
        got[pb] = (vol.clone(), counts, pos)
    assert torch.equal(got[0][0], got[1][0]) and got[0][1:] == got[1][1:]


def test_counters_same_nodes_fewer_pairs():
    """the mechanism: the walk is the same walk (node visits identical), the leaf pairs offered are the same, strictly fewer are
    tested.  The CPU model of the same walk on the same tree (tools/pair_box_model.py, a sample of the packets) is printed next to
    the GPU's ratio; nothing tighter than "fewer" is asserted."""
    st = {}
    for pb in (0, 1):
        m = mesh_handle("body", pb)
        st[pb] = m.pair_stats(65)
        m.close()
    v, f, _, _ = mesh("body")
    mod = model.model(model.Tree(v, f), 65, packets=40, seed=0)
    print(f"\npair_box off: {st[0]}\npair_box on:  {st[1]}\n"
          f"GPU pairs tested / offered: {st[1]['pairs_tested'] / st[1]['pairs_offered']:.3f}; "
          f"model (40 packets): {mod['boxed'] / mod['offered']:.3f} ({mod['offered']:.1f} offered, {mod['boxed']:.1f} tested per packet)")
    assert st[0]["packets"] == st[1]["packets"] > 0
    assert st[0]["nodes"] == st[1]["nodes"] and st[0]["pairs_offered"] == st[1]["pairs_offered"]
    assert st[0]["pairs_tested"] == st[0]["pairs_offered"]
    assert st[1]["pairs_tested"] < st[0]["pairs_tested"]

"""The restated loop of the packet walk (geom_device.h: nearest_packet - two descent loops and a leaf visit, records at 32-bit byte
offsets, the child choice on vote bits) on the GPU: it moves instructions and addresses, never a bit of a
result and never a visit.  Everything is compared with tests/golden/walk_scalar_parent.npz, recorded by
tools/make_golden_walk_scalar.py at the commit before the change: SHA-256 digests of the outputs and the walk's counters.
  - occupancy volumes at 33^3 (a trimmed tiling that ends in partial packets: parked lanes) and 65^3, body and sphere, both cmap
    modes: every lattice point's nearest slot, d^2 inside the clip band and sign (the library exposes the search's slot words and
    squared distances only through what is computed from them)
  - query() on 100,352 body points; point queries on the body, the 3,000 duplicate triangles (the lowest face index must still
    win) and the sliver mesh
  - the counters of icon_debug_walk_stats / icon_debug_pair_stats at 33^3 and 65^3: nodes, oriented visits, leaves, pairs offered
    and tested
  - a root that is a leaf of 1, 2, 3, 4 triangles, one inner node over two leaves (5 .. 8 triangles), a closed leaf (tetrahedron)
  - "pair_box" off, "node_box" off, both off, set before the mesh is created (the walk without its tables: the lattice
    launch is then the kernel that asks the mesh record at every visit)
  - 4,096 points 5 - 50 units outside the cube; bvh equals brute on the 33^3 points
share_waves = 1 makes the small lattices run k_nearest<lattice> itself, the kernel of the 257^3 call."""
import numpy as np
import pytest
import torch

from common import golden, set_option
import walk_scalar_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    g = golden("walk_scalar_parent.npz")
    return dict(zip((str(k) for k in g["names"]), (str(v) for v in g["values"])))


@pytest.fixture(autouse=True)
def options():
    set_option("share_waves", 1)
    yield
    set_option("share_waves", -1)
    set_option("pair_box", 1)
    set_option("node_box", 1)


def check(got, parent):
    assert got
    for k, v in got.items():
        print(f"{k}: {v}  (parent {parent.get(k)})")
    bad = [k for k, v in got.items() if str(v) != parent.get(k)]
    assert not bad, bad


def test_the_fixture_covers_every_case(parent):
    """nothing recorded that is no longer compared, nothing compared that was not recorded: the groups below are cases.GROUPS"""
    assert len(parent) > 100 and all(k.split("/")[0] in ("vol", "query", "points", "walk", "small", "switch", "far") for k in parent)
    assert {fn.__name__ for fn, _ in cases.GROUPS} == {"volumes", "query_body", "point_queries", "walk_counters", "small_mesh", "switched", "far"}


@pytest.mark.parametrize("cmap_mode", ["reference", "local"])
@pytest.mark.parametrize("name", ["body", "ico"])
def test_volumes(parent, name, cmap_mode):
    check(cases.volumes(name, cmap_mode), parent)


def test_query_on_body_points(parent):
    check(cases.query_body(), parent)


@pytest.mark.parametrize("name", ["body", "dup", "line"])
def test_point_queries(parent, name):
    check(cases.point_queries(name), parent)


@pytest.mark.parametrize("res", [33, 65])
def test_walk_counters_are_exactly_the_parents(parent, res):
    got = cases.walk_counters(res)
    assert got[f"walk/body/{res}/oriented_nodes"] > 0 and got[f"walk/body/{res}/pairs_tested"] < got[f"walk/body/{res}/pairs_offered"]
    check(got, parent)


@pytest.mark.parametrize("name", cases.SMALL)
def test_small_meshes(parent, name):
    got = cases.small_mesh(name)
    if name in ("strip1", "strip2", "strip3", "strip4", "tiny"):     # the root is a leaf: no inner node, every packet visits that leaf
        assert got[f"small/{name}/nodes"] == 0 and got[f"small/{name}/leaves"] == got[f"small/{name}/packets"] > 0
    else:                                                            # every packet visits the root, an inner node
        assert got[f"small/{name}/nodes"] >= got[f"small/{name}/packets"] > 0 and got[f"small/{name}/leaves"] > 0
    if name == "strip5":                                             # ... the only one (tests/test_gpu_node_box.py)
        assert got["small/strip5/nodes"] == got["small/strip5/packets"] and got["small/strip5/leaves"] <= 2 * got["small/strip5/packets"]
    check(got, parent)


@pytest.mark.parametrize("case", list(cases.SWITCHES))
def test_walk_without_its_tables(parent, case):
    got = cases.switched(case)
    pb, nb = cases.SWITCHES[case]
    assert (got[f"switch/{case}/oriented_nodes"] > 0) == bool(nb)
    assert (got[f"switch/{case}/pairs_tested"] < got[f"switch/{case}/pairs_offered"]) == bool(pb)
    check(got, parent)
    # whatever the tables, the same nearest faces and distances
    for k in ("vol33", "face", "sdf"):
        assert got[f"switch/{case}/{k}"] == parent[f"switch/both_on/{k}"], k


def test_far_points(parent):
    check(cases.far(), parent)


def test_bvh_search_equals_brute_force_at_33():
    """the lattice's own points, as a point query: the packet walk against the brute-force search, face and sdf bit for bit"""
    pts = cases.T(cases.lattice_points(33))
    m = cases.mesh_handle("body")
    b, w = m.sdf_query(pts, search="brute"), m.sdf_query(pts)
    m.close()
    for k in ("face", "sdf"):
        assert torch.equal(w[k], b[k]), k
    assert len(np.unique(w["face"].cpu().numpy())) > 100

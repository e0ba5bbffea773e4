"""The garment-extraction rule on the CPU: tests/garment_oracle.py - what the device is held to by equality in
tests/test_gpu_garment.py - against matplotlib's Path.contains_points, sklearn's KNeighborsClassifier(n_neighbors=1), the
reference's own extract_cloth (loaded from the reference tree where it exists, behind a stand-in trimesh container defined
here) and the stored run of that function (tests/golden/extract_cloth_ref.npz, written by tests/make_garment_golden.py); the host
helpers of icon_amd.garment against the oracle's, the reference's lists and tests/golden/smpl_part_labels.npz; and every argument
error that needs no device."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest

import garment_cases as gc
import garment_oracle as go
from common import ROOT, golden

# apps/infer.py:576-585
K_INFER = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -0.5, 0.0], [-0.0, -0.0, 0.5, 1.0]]).T
R_INFER = np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])
T_INFER = np.array([[-0.0, -0.0, 100.0]])


# ---- the stand-in for trimesh: the three members extract_cloth uses, restated -------------------------------------------------
class Trimesh:
    """Trimesh(vertices, faces) WITHOUT trimesh's process=True merge of coincident vertices (unpinned)"""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)

    def update_faces(self, mask):
        self.faces = self.faces[np.asarray(mask)]

    def remove_unreferenced_vertices(self):
        used = np.zeros(len(self.vertices), dtype=bool)
        used[self.faces.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        self.vertices, self.faces = self.vertices[used], remap[self.faces]


def reference_root():
    from oracle import ref_loader
    return ref_loader.REFERENCE_ROOT


def load_reference():
    """the reference's lib/common/cloth_extraction.py, imported from where it lies with `trimesh` bound to the stand-in; None
    where the tree, matplotlib or sklearn is absent"""
    path = os.path.join(reference_root(), "lib", "common", "cloth_extraction.py")
    if not os.path.isfile(path):
        return None
    try:
        import matplotlib.path  # noqa: F401
        import sklearn.neighbors  # noqa: F401
    except ImportError:
        return None
    stand_in = types.ModuleType("trimesh")
    stand_in.Trimesh = Trimesh
    saved = sys.modules.get("trimesh")
    sys.modules["trimesh"] = stand_in
    try:
        spec = importlib.util.spec_from_file_location("_reference_cloth_extraction", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules["trimesh"]
        else:
            sys.modules["trimesh"] = saved
    return mod


def reference_part_table():
    path = os.path.join(reference_root(), "lib", "common", "smpl_vert_segmentation.json")
    if not os.path.isfile(path):
        return None
    with open(path) as fh:
        return json.load(fh)


def golden_case():
    """inputs of the stored run: the reconstruction stand-in (a noisy ellipsoid around the synthetic body), the synthetic body as
    the SMPL mesh, two overlapping polygons in normalised image coordinates"""
    from icon_amd import synth
    rng = np.random.RandomState(1907)
    nu, nv = 48, 64
    u, v = np.meshgrid(np.linspace(0.02, np.pi - 0.02, nu), np.linspace(0, 2 * np.pi, nv, endpoint=False), indexing="ij")
    r = 1.0 + 0.05 * rng.standard_normal(u.shape)
    verts = np.stack([0.5 * r * np.sin(u) * np.cos(v), -0.05 + 0.92 * r * np.cos(u), 0.2 * r * np.sin(u) * np.sin(v)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv), indexing="ij")
    a, b, c, d = i * nv + j, i * nv + (j + 1) % nv, (i + 1) * nv + j, (i + 1) * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    body, body_faces = synth.load_body_mesh()
    torso = np.array([[-0.31, 0.52], [-0.12, 0.61], [0.0, 0.5], [0.13, 0.6], [0.3, 0.53], [0.37, 0.2], [0.24, 0.13], [0.27, -0.33],
                      [0.0, -0.41], [-0.26, -0.3], [-0.22, 0.1], [-0.39, 0.22]])
    patch = np.array([[0.1, 0.3], [0.45, 0.45], [0.5, -0.1], [0.3, -0.5], [0.05, -0.2]])
    # model plane -> normalised image coordinates: the inverse of the (diagonal) map polygons_to_model_plane applies
    scale = go.polygons_to_model_plane([np.array([[1.0, 1.0], [0.0, 0.0]])], K_INFER, R_INFER, T_INFER)[0][0]
    coords = [torso / scale, patch / scale]
    return dict(verts=verts, faces=faces, body=np.ascontiguousarray(body, dtype=np.float32), body_faces=np.asarray(body_faces), coords=coords)


def stored_case():
    """the inputs of the stored run as the fixture holds them (no libm between the recording and the reading); the body from synth"""
    from icon_amd import synth
    g = golden("extract_cloth_ref.npz")
    body, body_faces = synth.load_body_mesh()
    coords = [g[f"coords_{k}"] for k in range(sum(1 for n in g.files if n.startswith("coords_")))]
    return dict(verts=g["verts"], faces=g["faces"], body=np.ascontiguousarray(body, dtype=np.float32), body_faces=np.asarray(body_faces), coords=coords)


def reference_labels(ref, n_verts=6890):
    """the part name of every SMPL vertex as the reference's OWN smpl_to_recon_labels assigns it: n_verts distinct points labelled
    from themselves - every point is its own nearest neighbour, so the prediction is the table the function built -> (names, int8)"""
    pts = np.stack([np.arange(n_verts, dtype=np.float64), np.zeros(n_verts), np.zeros(n_verts)], 1)
    by_part = ref.smpl_to_recon_labels(_Mesh(pts, None), _Mesh(pts, None))
    names = list(by_part.keys())
    labels = np.full(n_verts, -1, dtype=np.int8)
    for k, name in enumerate(names):
        labels[np.asarray(by_part[name], dtype=np.int64)] = k
    assert (labels >= 0).all()
    return names, labels


GOLDEN_TYPES = (1, 2, 5, 7)               # one of each removal list: forearms, base only, + arms, + lower legs


class _Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


# ---- rule 2 against matplotlib ---------------------------------------------------------------------------------------------------
def _polygon_cases():
    rng = np.random.RandomState(5)
    cases = [("random", gc.star_polygon(rng, n)) for n in (3, 4, 5, 7, 12, 23, 41, 60)]
    cases += [("lattice", gc.lattice_polygon(rng, n)) for n in (3, 4, 6, 9, 17, 33, 60)]
    cases += [("one", np.array([[0.25, 0.25]])), ("two", np.array([[-0.5, -0.5], [0.5, 0.5]])), ("tangle", gc.tangle_polygon(rng, 9)),
              ("tangle-lattice", np.round(gc.tangle_polygon(rng, 14) * 8) / 8)]
    return cases


def test_oracle_containment_is_matplotlibs():
    mpath = pytest.importorskip("matplotlib.path", reason="matplotlib is not installed: the crossings rule cannot be pinned here")
    rng = np.random.RandomState(6)
    inside = total = 0
    for name, poly in _polygon_cases():
        pts = gc.mixed_points(rng, 20000)
        pts[:len(poly)] = poly                                                   # the polygon's own vertices
        pts[len(poly):2 * len(poly)] = 0.5 * (poly + np.roll(poly, -1, 0))          # edge midpoints (exact on the lattice)
        for p in (pts, pts.astype(np.float32)):                                  # float32 points are what the device widens
            want = mpath.Path(poly).contains_points(p)
            got = go.contains(poly, p)
            assert np.array_equal(got, want), f"{name} polygon of {len(poly)}: {int((got != want).sum())} of {len(p)} points differ"
            inside += int(got.sum()); total += len(p)
        if len(poly) < 3:
            assert not go.contains(poly, pts).any()
    assert 0.1 < inside / total < 0.9                                            # not a comparison of all-false with all-false


def test_oracle_nearest_labels_are_sklearns():
    nb = pytest.importorskip("sklearn.neighbors", reason="scikit-learn is not installed: the nearest-vertex rule cannot be pinned here")
    rng = np.random.RandomState(7)
    src = rng.uniform(-1, 1, (6890, 3)).astype(np.float32)
    src[100:110] = src[90:100]                                                   # duplicated source vertices: ties
    labels = rng.randint(0, 24, 6890)
    labels[100:110] = labels[90:100]            # ... under one label: which of two coincident points sklearn's k-d tree returns is its own affair
    q = rng.uniform(-1, 1, (20000, 3)).astype(np.float32)
    q[:10] = src[100:110]                                                        # queries ON the duplicated vertices
    want = nb.KNeighborsClassifier(n_neighbors=1).fit(src, labels).predict(q)
    nn = go.nearest(q, src)
    assert np.array_equal(labels[nn], want)
    assert np.array_equal(nn[:10], np.arange(90, 100))                            # the lowest index of a tie
    brute = np.array([((q[i].astype(np.float64) - src.astype(np.float64)) ** 2).sum(-1).argmin() for i in range(200)])
    assert np.array_equal(nn[:200], brute)


# ---- the whole rule against the reference's function ------------------------------------------------------------------------------
def _oracle_run(case, type_id, table):
    names, labels = go.part_labels(table, len(case["body"])) if isinstance(table, dict) else table
    remove = np.isin(labels, [names.index(p) for p in go.parts_to_remove(type_id)])
    polys = go.polygons_to_model_plane(case["coords"], K_INFER, R_INFER, T_INFER)
    return go.extract(case["verts"], case["faces"], polys, case["body"], remove)


def test_oracle_is_the_reference_function():
    ref, table = load_reference(), reference_part_table()
    if ref is None or table is None:
        pytest.skip("the reference tree (or matplotlib / scikit-learn) is not here; test_oracle_is_the_stored_run covers the same ground")
    case = golden_case()
    sizes = set()
    for type_id in range(1, 14):
        mesh = ref.extract_cloth(_Mesh(case["verts"], case["faces"]), dict(coord_normalized=case["coords"], type_id=type_id),
                                 K_INFER, R_INFER, T_INFER, _Mesh(case["body"], case["body_faces"]))
        o = _oracle_run(case, type_id, table)
        gc.not_vacuous(o)
        assert mesh is not None and np.array_equal(mesh.vertices, o["verts"]) and np.array_equal(mesh.faces, o["faces"]), f"type_id {type_id}"
        sizes.add((len(o["verts"]), len(o["faces"])))
    assert len(sizes) >= 3                                                       # the removal lists make a difference


def test_oracle_is_the_stored_run():
    g, lab = golden("extract_cloth_ref.npz"), golden("smpl_part_labels.npz")
    case = stored_case()
    assert case["verts"].shape == (3072, 3) and case["verts"].dtype == np.float32 and len(case["coords"]) == 2
    table = ([str(n) for n in lab["names"]], lab["labels"].astype(np.int32))
    for type_id in GOLDEN_TYPES:
        o = _oracle_run(case, type_id, table)
        gc.not_vacuous(o)
        assert np.array_equal(g[f"out_verts_{type_id}"], o["verts"]) and np.array_equal(g[f"out_faces_{type_id}"], o["faces"]), f"type_id {type_id}"


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------
def test_part_labels_and_removal_lists():
    from icon_amd import garment as gm
    lab = golden("smpl_part_labels.npz")
    names, labels = [str(n) for n in lab["names"]], lab["labels"]
    assert len(names) == 24 and labels.shape == (6890,) and labels.dtype == np.int8 and labels.min() == 0 and labels.max() == 23
    table = reference_part_table()
    if table is not None:                                                         # the fixture is the reference's rule on its JSON
        n2, l2 = gm.part_labels(table, 6890)
        assert n2 == names and l2.dtype == np.int32 and np.array_equal(l2, labels)
        n3, l3 = go.part_labels(table, 6890)
        assert n3 == names and np.array_equal(l3, labels)
        ref = load_reference()
        if ref is not None:                                                       # ... and what the reference's own function assigns
            n5, l5 = reference_labels(ref)
            assert n5 == names and np.array_equal(l5, labels)
        assert sum(len(v) for v in table.values()) - 6890 == 500                  # the doubly-listed vertices: the later key wins
    # a table rebuilt from the fixture gives the fixture back
    rebuilt = {n: np.nonzero(labels == k)[0].tolist() for k, n in enumerate(names)}
    n4, l4 = gm.part_labels(rebuilt, 6890)
    assert n4 == names and np.array_equal(l4, labels)
    base = ["rightHand", "leftToeBase", "leftFoot", "rightFoot", "head", "leftHandIndex1", "rightHandIndex1", "rightToeBase", "leftHand", "rightHand"]
    for t in range(0, 15):
        got = gm.parts_to_remove(t)
        assert got == go.parts_to_remove(t) and got[:10] == base and set(got) <= set(names)
        extra = got[10:]
        if t in (1, 3, 10):
            assert extra == ["leftForeArm", "rightForeArm"]
        elif t in (5, 6, 8, 9, 12, 13):
            assert extra == ["leftForeArm", "rightForeArm", "leftArm", "rightArm"]
        elif t == 7:
            assert extra == ["leftLeg", "rightLeg", "leftForeArm", "rightForeArm", "leftArm", "rightArm"]
        else:
            assert extra == []


def test_polygons_to_model_plane():
    from icon_amd import garment as gm
    rng = np.random.RandomState(8)
    coords = [rng.uniform(-0.02, 0.02, (n, 2)) for n in (3, 1, 40)]
    for K, R, t in ((K_INFER, R_INFER, T_INFER), (K_INFER + 0.01 * rng.standard_normal((4, 4)), R_INFER, T_INFER.reshape(3))):
        got, want = gm.polygons_to_model_plane(coords, K, R, t), go.polygons_to_model_plane(coords, K, R, t)
        assert all(a.dtype == np.float64 and a.tobytes() == b.tobytes() for a, b in zip(got, want))
    # apps/infer.py's matrices: a reflection of x and a scale
    xy = gm.polygons_to_model_plane([np.array([[0.01, 0.0], [0.0, 0.01]])], K_INFER, R_INFER, T_INFER)[0]
    assert xy[0, 0] > 0.4 and abs(xy[0, 1]) < 1e-12 and xy[1, 1] < -0.4 and abs(xy[1, 0]) < 1e-12


def test_argument_errors():
    import torch
    from icon_amd import garment as gm
    from icon_amd._lib import IconAmdError
    v, f = torch.zeros(10, 3), torch.zeros(4, 3, dtype=torch.int64)
    tri = [np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])]

    def refused(match, fn, *a, **k):
        with pytest.raises(IconAmdError, match=match):
            fn(*a, **k)

    refused("verts must be \\[N,3\\]", gm.extract_cloth_device, torch.zeros(10, 2), f, tri)
    refused("verts must be a floating-point", gm.extract_cloth_device, torch.zeros(10, 3, dtype=torch.int32), f, tri)
    refused("verts must be a tensor", gm.extract_cloth_device, np.zeros((10, 3)), f, tri)
    refused("faces must be an integer", gm.extract_cloth_device, v, f.float(), tri)
    refused("faces must be \\[F,3\\]", gm.extract_cloth_device, v, torch.zeros(4, 4, dtype=torch.int64), tri)
    refused("src_remove given without src_verts", gm.extract_cloth_device, v, f, tri, None, torch.zeros(5, dtype=torch.bool))
    refused("src_verts given without src_remove", gm.extract_cloth_device, v, f, tri, torch.zeros(5, 3))
    refused("src_verts must be \\[N,3\\]", gm.extract_cloth_device, v, f, tri, torch.zeros(5, 4), torch.zeros(5, dtype=torch.bool))
    refused("src_remove must be a bool or uint8", gm.extract_cloth_device, v, f, tri, torch.zeros(5, 3), torch.zeros(5))
    refused("src_remove must be \\[Vs\\]", gm.extract_cloth_device, v, f, tri, torch.zeros(5, 3), torch.zeros(6, dtype=torch.bool))
    refused("polygon 0 must be \\[n,2\\]", gm.extract_cloth_device, v, f, [np.zeros((3, 3))])
    refused("polygon 1 has a coordinate that is not finite", gm.extract_cloth_device, v, f, tri + [np.array([[0.0, np.nan], [1.0, 0.0], [0.0, 1.0]])])
    refused("polygon 0 has a coordinate that is not finite", gm.extract_cloth_device, v, f, [np.array([[0.0, np.inf], [1.0, 0.0], [0.0, 1.0]])])
    refused("polygon 0 must hold numbers", gm.extract_cloth_device, v, f, [np.array([["a", "b"]])])
    refused("verts must be \\[N,3\\]", gm.nearest_vertex_device, torch.zeros(3), torch.zeros(5, 3))
    refused("src_verts must be \\[N,3\\]", gm.nearest_vertex_device, v, torch.zeros(5, 2))
    refused("src_verts is empty", gm.nearest_vertex_device, v, torch.zeros(0, 3))
    refused("only must be \\[10\\]", gm.nearest_vertex_device, v, torch.zeros(5, 3), torch.zeros(9, dtype=torch.bool))
    refused("only must be a bool or uint8", gm.nearest_vertex_device, v, torch.zeros(5, 3), torch.zeros(10))
    refused("src_labels must be a tensor \\[Vs\\]", gm.transfer_labels_device, v, torch.zeros(5, 3), torch.zeros(4, dtype=torch.int64))
    if not torch.cuda.is_available():                                             # host tensors where a device is needed: no CPU path
        refused("needs the HIP device", gm.extract_cloth_device, v, f, tri)
        refused("needs the HIP device", gm.nearest_vertex_device, v, torch.zeros(5, 3))
    # the reference's entry point
    seg = dict(coord_normalized=[tri[0] / 50.0], type_id=1)
    mesh = (np.zeros((10, 3), np.float32), np.zeros((4, 3), np.int64))
    refused("segmentation must be a dict", gm.extract_cloth, mesh, None, K_INFER, R_INFER, T_INFER)
    refused("segmentation must be a dict", gm.extract_cloth, mesh, dict(type_id=1), K_INFER, R_INFER, T_INFER)
    refused("recon must have .vertices and .faces", gm.extract_cloth, 3, seg, K_INFER, R_INFER, T_INFER)
    refused("recon vertices must be \\[N,3\\]", gm.extract_cloth, (np.zeros((10, 2), np.float32), mesh[1]), seg, K_INFER, R_INFER, T_INFER)
    refused("recon faces must be an integer \\[F,3\\]", gm.extract_cloth, (mesh[0], np.zeros((4, 3), np.float32)), seg, K_INFER, R_INFER, T_INFER)
    refused("K must be at least \\[3,3\\]", gm.extract_cloth, mesh, seg, np.eye(2), R_INFER, T_INFER)
    refused("polygon 0 must be \\[n,2\\]", gm.extract_cloth, mesh, dict(coord_normalized=[np.zeros((3, 3))], type_id=1), K_INFER, R_INFER, T_INFER)
    refused("not finite in the model plane", gm.extract_cloth, mesh, dict(coord_normalized=[np.array([[np.nan, 0.0]])]), K_INFER, R_INFER, T_INFER)
    refused("smpl given without vert_segmentation", gm.extract_cloth, mesh, seg, K_INFER, R_INFER, T_INFER, smpl=mesh)
    lab = golden("smpl_part_labels.npz")
    names = [str(n) for n in lab["names"]]
    refused("labels must be \\[10\\]", gm.extract_cloth, mesh, seg, K_INFER, R_INFER, T_INFER, smpl=mesh, vert_segmentation=(names, lab["labels"]))
    refused("the part table has no", gm.extract_cloth, mesh, seg, K_INFER, R_INFER, T_INFER, smpl=mesh,
            vert_segmentation=(["a", "b"], np.zeros(10, np.int32)))
    refused("has no 'type_id'", gm.extract_cloth, mesh, dict(coord_normalized=seg["coord_normalized"]), K_INFER, R_INFER, T_INFER, smpl=mesh,
            vert_segmentation=(names, np.zeros(10, np.int32)))
    refused("face index out of range", gm.extract_cloth, (mesh[0], np.full((4, 3), 10, np.int64)), seg, K_INFER, R_INFER, T_INFER)
    refused("face index out of range", gm.extract_cloth, (mesh[0], np.full((4, 3), -1, np.int64)), seg, K_INFER, R_INFER, T_INFER)
    # the part table
    refused("vert_segmentation must be a non-empty dict", gm.part_labels, [], 4)
    refused("names vertex 4", gm.part_labels, dict(a=[0, 1], b=[2, 4]), 4)
    refused("names vertex -1", gm.part_labels, dict(a=[0, 1], b=[2, -1]), 4)
    refused("1 vertices are in no part \\(the first: 3\\)", gm.part_labels, dict(a=[0, 1], b=[2]), 4)
    refused("must list integer vertex indices", gm.part_labels, dict(a=[0.5]), 4)


def test_tile_constants_agree():
    """the tile sizes the GPU tests pick their shapes around are the kernel's"""
    from icon_amd import garment as gm
    src = open(os.path.join(ROOT, "icon_amd", "csrc", "garment.hip")).read()
    assert f"constexpr int kPolyTile = {gm.POLY_TILE};" in src and f"constexpr int kSrcTile = {gm.SRC_TILE};" in src
    assert "constexpr int kSrcSplit = kSrcTile / 4;" in src and gm.SRC_SPLIT * 4 == gm.SRC_TILE
    src = open(os.path.join(ROOT, "icon_amd", "csrc", "compact_device.h")).read()
    assert "constexpr int kCompactBlock = 256;" in src and "constexpr int kCompactRound = 8192;" in src and gm.SCAN_ROUND == 8192 * 256
